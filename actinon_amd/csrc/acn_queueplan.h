/* acn_queueplan.h -- the planning arithmetic of the pipeline runner (actinon_hip.hip) as plain host C, next to acn_chunkplan.h:
 * queue capacities, chunk sizes, learned rates, the reading of a chunk's counter blocks (acn_counts.h), walk passes, lanes and the
 * tile order.  No HIP header: capacities, rates, record sizes and the copied counter blocks come in as arguments and the decisions
 * go out, so every rule runs without a GPU (tests/csrc/queueplan_cpu.cpp, tests/test_queueplan_cpu.py).  Compiled by two compilers:
 * keep -ffp-contract=off. */
#ifndef ACN_QUEUEPLAN_H
#define ACN_QUEUEPLAN_H

#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include "acn_counts.h"

/* the queues of a pipeline run.  Each is sized from its OWN demand per sample position (learned, below): on the wine glass a
 * position leaves 15 deferred shadow rays but 2 shading points, and one common capacity -- the former layout -- made every
 * queue as large as the fullest one needs (64 GiB for a 1080p frame of which 7 % were used). */
enum { WQ_TASKS = 0, WQ_CHILDREN, WQ_HARD_SHADOW, WQ_HARD_PATH, WQ_RAYS, WQ_N };

#define ACN_CHUNK_TARGET ( ( size_t )1 << 22 )
#define ACN_STARTER_RECORDS ( ( size_t )1 << 20 )
#define ACN_LANE_TILE 256

static inline double acn_plan_max( double a, double b ) { return a > b ? a : b; }
static inline int acn_rates_known( const double* rate ) { return rate[ WQ_TASKS ] > 0 || rate[ WQ_RAYS ] > 0 || rate[ WQ_HARD_SHADOW ] > 0; }
/* records per position a queue of the current call needs: the learned rate, and in the ray queue of a ray call at least one
 * slot per position whatever earlier calls taught the handle -- its seeded generation is a KNOWN demand, kept out of the
 * learned rates (acn_read_chunk) */
static inline double acn_queue_demand( const double* rate, int q, int seeded ) { return seeded && q == WQ_RAYS && rate[ q ] < 1.0 ? 1.0 : rate[ q ]; }

/* positions a chunk may have so that every queue stays below fill_target (70 %) of its capacity */
static inline size_t acn_chunk_for_caps( const double* rate, int seeded, double fill_target, const uint32_t* cap )
{
    double chunk = 2.0e9;
    for( int q = 0; q < WQ_N; q++ )
    {
        const double r = acn_queue_demand( rate, q, seeded ) > 1e-3 ? acn_queue_demand( rate, q, seeded ) : 1e-3;
        const double c = fill_target * ( double )cap[ q ] / r;
        if( c < chunk ) chunk = c;
    }
    return chunk < 64 ? 64 : ( size_t )chunk;
}

/* Positions the starter queues hold before anything is learned, `most` at most: a guess that errs on the safe side by factors,
 * not orders of magnitude (an overflow costs one small chunk): path-sample hits ~ path_samples per position, squared from 64
 * samples on (two nested levels); a quarter of the direct-light samples deferred.  most: 32 768 for a first chunk. */
static inline size_t acn_first_chunk_guess( uint32_t cap_children, uint32_t cap_hard_shadow, uint64_t path_samples, uint64_t direct_samples,
                                            size_t n_lights, size_t most )
{
    const size_t s = path_samples ? path_samples : 1;
    size_t want = ( size_t )( ( double )cap_children / ( ( double )( s + 2 ) * ( s > 64 ? ( double )s / 64.0 : 1.0 ) ) );
    const size_t by_shadow = ( size_t )( ( double )cap_hard_shadow / ( 0.25 * ( double )( direct_samples * n_lights + s ) + 4.0 ) );
    if( want > by_shadow ) want = by_shadow;
    if( want > most ) want = most;
    return want;
}
/* ... and of the learning sample of n positions: 4096 at most.  (The guess is ten times what the lamp scenes need at path_samples
 * 1024, where it allowed 63 positions: no sample at all, and the whole hanging_lamp frame at stated size began every band with
 * ~20 redone chunks, halving down from 92 000 positions to 9.  A sample that does not fit is halved by learn_rates.) */
static inline size_t acn_sample_positions( uint32_t cap_children, uint32_t cap_hard_shadow, uint64_t path_samples, uint64_t direct_samples,
                                           size_t n_lights, size_t n )
{
    size_t want = acn_first_chunk_guess( cap_children, cap_hard_shadow, path_samples, direct_samples, n_lights, 4096 );
    if( want < 256 ) want = 256;
    if( want > n / 4 ) want = n / 4;
    return want;
}

/* Queue capacities.  Only one chunk of positions is in flight per pipeline run, so the queues are sized for a chunk, not
 * for the call, and each queue for its own demand:
 *   - rates unknown (first call on a handle): a small uniform starter set, 2^20 records per queue (the deferred-shadow queue
 *     twice that), less for a call of a few positions; the first chunk of the call is small, teaches the rates (render_chunk)
 *     and launch_render comes back here;
 *   - rates known: room for as many positions as the call has (at most ACN_CHUNK_TARGET) at 1 / 0.7 of the learned rates,
 *     scaled down to the budget (ACN_WORKSPACE_MB; default 64 GiB or a quarter of the free device memory) less the stacks if
 *     that is less.  The chunk size follows the capacities (launch_render), so a small workspace costs more chunks, not
 *     correctness; if hipMalloc refuses, the request is halved until it fits (acn_halve_caps).
 * rec_bytes: bytes per record of each queue */
static inline void acn_wanted_caps( const double* rate, int seeded, size_t n, uint64_t path_samples, uint64_t direct_samples, size_t n_lights,
                                    size_t budget, size_t stack_bytes, const size_t* rec_bytes, size_t* want )
{
    if( !acn_rates_known( rate ) )
    {
        const size_t s = path_samples ? path_samples : 1;
        const size_t per_pos = ( s + 2 ) * ( s > 16 ? s / 16 : 1 ) + ( size_t )direct_samples * n_lights;
        size_t recs = n * per_pos + 65536;
        if( recs > ACN_STARTER_RECORDS ) recs = ACN_STARTER_RECORDS;
        size_t per_rec = rec_bytes[ WQ_HARD_SHADOW ];
        for( int q = 0; q < WQ_N; q++ ) per_rec += rec_bytes[ q ];
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
        for( int q = 0; q < WQ_N; q++ ) bytes += ( slack * acn_queue_demand( rate, q, seeded ) * positions / 0.7 + 65536.0 ) * ( double )rec_bytes[ q ];
        const double room = budget > stack_bytes ? ( double )( budget - stack_bytes ) : 0.0;
        if( bytes > room ) positions *= room / bytes;
        for( int q = 0; q < WQ_N; q++ )
        {
            double c = slack * acn_queue_demand( rate, q, seeded ) * positions / 0.7 + 65536.0;
            want[ q ] = c > 4.0e9 ? 0xFFFFFF00ull : ( size_t )c;
        }
    }
    for( int q = 0; q < WQ_N; q++ ) { if( want[ q ] < 65536 ) want[ q ] = 65536; if( want[ q ] > 0xFFFFFF00ull ) want[ q ] = 0xFFFFFF00ull; }
}

/* 1: the queues stay as they are.  They do while they hold what the rates ask for (the slack is for growth, not a reason to
 * re-allocate) ... and give back what the first, small chunks of a handle over-estimated (their dead slots do not scale): once
 * (*trim, for Workspace::trimmed), when the rates come from a large chunk and the queues hold 40 % more than those ask for (slack
 * included) ... in a WINDOW: the first few sizing steps after the rates were learned (the second and third call of a handle;
 * *sized_calls counts them).  Rates decay slowly towards what the chunks really leave, so without the window the condition could
 * first become true ten frames later and put 100 ms of hipFree + hipMalloc into an arbitrary frame (round 4, session 10: the
 * 1080p bench line read 68.6 ms instead of 51.8 because the trim fell into its ten timed steps) */
static inline int acn_keep_caps( const uint32_t* cap, size_t have_stack_waves, size_t stack_waves, const size_t* want, const size_t* rec_bytes,
                                 int known, uint32_t rate_cnt, int trimmed, uint32_t* sized_calls, int* trim )
{
    *trim = 0;
    int fits = have_stack_waves >= stack_waves;
    for( int q = 0; q < WQ_N; q++ ) if( ( double )cap[ q ] < ( double )want[ q ] / 1.4 ) fits = 0;
    if( known && rate_cnt >= 32768 ) ( *sized_calls )++;
    if( fits && known && rate_cnt >= 32768 && !trimmed && *sized_calls <= 3 )
    {
        size_t have = 0, need = 0;
        for( int q = 0; q < WQ_N; q++ ) { have += ( size_t )cap[ q ] * rec_bytes[ q ]; need += want[ q ] * rec_bytes[ q ]; }
        if( ( double )have > 1.25 * ( double )need && have - need > ( ( size_t )1 << 29 ) ) { fits = 0; *trim = 1; }
    }
    return fits;
}
/* hipMalloc refused: half of everything, 65536 records at least.  1: it was the floor already */
static inline int acn_halve_caps( size_t* want )
{
    int floor = 1;
    for( int q = 0; q < WQ_N; q++ ) { if( want[ q ] > 65536 ) floor = 0; want[ q ] = want[ q ] / 2 < 65536 ? 65536 : want[ q ] / 2; }
    return floor;
}

/* ---- the rates: records per sample position a chunk leaves in each queue ---- */
/* ... from the queue marks of one chunk of cnt positions.  (A chunk of a few positions: mostly dead slots, 64 positions of
 * hanging_lamp p1024 mark 15 600 deferred rays per position where 3 500 is the rate -- the counted share of the deferred-shadow
 * queue corrects all five) */
static inline void acn_set_rates( double* rate, uint32_t* rate_cnt, uint32_t cnt, const uint32_t* fill, double dead_share )
{
    const double live = cnt <= 4096 && dead_share > 0 && dead_share < 0.95 ? 1.0 - dead_share : 1.0;
    for( int q = 0; q < WQ_N; q++ ) rate[ q ] = acn_plan_max( live * ( double )fill[ q ] / ( double )cnt, 1e-3 );
    *rate_cnt = cnt;
}
/* Learn from a chunk that fitted.  A chunk much larger than the one the rates came from replaces them (the dead slots at the ends
 * of the waves' queue reservations do not scale with the chunk, so small chunks over-estimate); otherwise the rates follow
 * upwards at once and forget slowly (also after small chunks: where chunks are small the demand per position is large and the
 * dead slots do not matter; rates that only went up left many_spheres p256 with 532 chunks of 3 900 positions after one spike) */
static inline void acn_learn_rates( double* rate, uint32_t* rate_cnt, uint32_t cnt, const uint32_t* fill, double dead_share )
{
    if( !acn_rates_known( rate ) || cnt >= 4 * *rate_cnt ) { acn_set_rates( rate, rate_cnt, cnt, fill, dead_share ); return; }
    for( int q = 0; q < WQ_N; q++ ) rate[ q ] = acn_plan_max( acn_plan_max( ( double )fill[ q ] / ( double )cnt, 0.85 * rate[ q ] ), 1e-3 );
    if( cnt > *rate_cnt ) *rate_cnt = cnt;
}
/* the marks of an overflowed chunk are lower bounds of its demand */
static inline void acn_overflow_rates( double* rate, uint32_t cnt, const uint32_t* fill )
{
    for( int q = 0; q < WQ_N; q++ ) { const double r = ( double )fill[ q ] / ( double )cnt; if( r > rate[ q ] ) rate[ q ] = r; }
}

/* The rates from the learning sample of cnt positions: the records the sample left in each queue, exactly (marks minus dead
 * slots; the fullest level counts, the queues are the levels' in turn), plus a fifth for what a sample of a few thousand
 * positions does not see.
 * What a queue must hold is records PLUS the slots that die at the ends of the waves' reservations: up to 64 per wave,
 * queue and launch that appends to it, whatever the chunk's size (a chunk of 230 000 positions of the wine glass marks 1.1 M
 * task slots for 0.45 M tasks).  The planner's rates are marks per position, so the dead slots of a chunk of the size the
 * call will run -- plan_positions, on persistent grids of plan_grid workgroups -- are spread over its positions:
 * tasks, specular rays and probes are appended by k_shade_hits and ~4 walk passes, path-sample hits and the two deferred
 * queues by the four k_shade launches (and k_hard_path). */
static inline void acn_sample_rates( const uint32_t* counts, int levels, uint32_t cnt, size_t plan_positions, unsigned plan_grid, double* rate )
{
    double live[ WQ_N ] = { 0, 0, 0, 0, 0 };
    for( int level = 0; level < levels; level++ )
    {
        const uint32_t* c = counts + ( size_t )level * QC_N;
#define ACN_UP( q, v ) do { const double v_ = ( v ); if( v_ > live[ q ] ) live[ q ] = v_; } while( 0 )
        ACN_UP( WQ_TASKS, ( double )c[ QC_TASKS ] - ( double )c[ QS_DEAD_T ] );
        ACN_UP( WQ_CHILDREN, ( double )c[ QC_CHILDREN ] - ( double )c[ QS_DEAD_C ] );
        ACN_UP( WQ_HARD_SHADOW, ( double )c[ QS_HARD_SHADOW ] + ( double )c[ QS_PROBES ] );
        ACN_UP( WQ_HARD_PATH, ( double )c[ QC_HARD_PATH ] - ( double )c[ QS_DEAD_HP ] );
        /* rays: no generation holds more than the largest mark, nor more than all the level's generations together */
        double sum = 0, top = 0;
        for( uint32_t g = 0; g < ACN_MAX_WALK_PASSES + 1; g++ ) { sum += c[ QC_GEN + g ]; if( c[ QC_GEN + g ] > top ) top = c[ QC_GEN + g ]; }
        sum -= ( double )c[ QS_DEAD_R ];
        ACN_UP( WQ_RAYS, sum < top ? sum : top );
#undef ACN_UP
    }
    const double per_launch = ( double )ACN_QCHUNK * 4.0 * ( double )plan_grid;
    const double walkers = 3.0 * per_launch, shaders = 3.0 * per_launch;   /* (not every wave of every launch leaves a full reservation behind) */
    const double dead[ WQ_N ] = { walkers, shaders, walkers + shaders, shaders, walkers };
    const double pp = ( double )( plan_positions < ACN_CHUNK_TARGET ? plan_positions : ACN_CHUNK_TARGET );
    /* a generation of specular rays is at most three children per shaded hit (path-sample hits of the level before, or the
     * camera rays' shading points): the sample's ray marks are mostly dead slots */
    const double ray_bound = 2.0 * live[ WQ_CHILDREN ] + live[ WQ_TASKS ];
    if( live[ WQ_RAYS ] > ray_bound && ray_bound > 0 ) live[ WQ_RAYS ] = ray_bound;
    for( int q = 0; q < WQ_N; q++ ) rate[ q ] = acn_plan_max( 1.2 * live[ q ] / ( double )cnt + dead[ q ] / pp, 1e-3 );
}

/* ---- a change of scene on a live handle (acn_scene_replace, acn_scene_set_params) ---- */
/* What the learned rates depend on.  They are records per POSITION, so the raster size is no part of it, nor is the camera: a frame
 * of the same kind from another angle leaves about the same records per position, and rates that are off cost a redone chunk, never
 * a pixel (a chunk that overflows is rendered again, bit-identically). */
typedef struct
{
    uint32_t n_nodes, n_elems;
    uint64_t n_lights;
    int32_t  n_levels, prune;
    uint64_t path_samples, direct_samples, trace_depth;
    double   trace_min_intensity;
} acn_scene_kind;
/* 1: the runners keep what they learned (rates, fill target, walk passes) across the change: iff every member is equal, the double by
 * its bit pattern (-0.0 is not 0.0: no rule about values, only "nothing changed") */
static inline int acn_replace_keeps_learned( const acn_scene_kind* was, const acn_scene_kind* now )
{
    uint64_t a, b;
    memcpy( &a, &was->trace_min_intensity, sizeof( a ) ); memcpy( &b, &now->trace_min_intensity, sizeof( b ) );
    return was->n_nodes == now->n_nodes && was->n_elems == now->n_elems && was->n_lights == now->n_lights && was->n_levels == now->n_levels &&
           was->prune == now->prune && was->path_samples == now->path_samples && was->direct_samples == now->direct_samples &&
           was->trace_depth == now->trace_depth && a == b;
}

/* ---- walk passes ---- */
/* launches of k_walk for path level `level`: ACN_WALK_PASSES (tun_passes), but no more than the hits of the level have depth left.
 * The chunks of a call see the same mix of pixels (TileOrder), so the passes that had input in the last chunk (seen; 0: not
 * known, or not to be used), plus one, are the passes this chunk needs: the last launch of a level finishes whatever is left on
 * the private stacks in any case, so a guess that is too low costs time, never rays.  (A frame without specular surfaces: 2
 * launches per level instead of 12.) */
static inline uint32_t acn_walk_passes( uint64_t trace_depth, int level, uint32_t tun_passes, uint32_t seen )
{
    const uint64_t depth_left = trace_depth > 10ull * ( uint64_t )level ? trace_depth - 10ull * ( uint64_t )level : 1;
    uint32_t passes = tun_passes;
    if( passes > depth_left + 1 ) passes = ( uint32_t )depth_left + 1;
    if( seen && seen + 1 < passes ) passes = seen + 1;
    return passes;
}
/* the passes of a level that had input, from its generation marks gen[ 0 .. launched ) */
static inline uint32_t acn_walk_passes_seen( const uint32_t* gen, uint32_t launched )
{
    uint32_t used = 1;   /* pass 0 of level 0 has the camera rays; a level without rays keeps one launch */
    for( uint32_t g = 0; g < launched; g++ ) if( gen[ g ] ) used = g + 1;
    /* the last launch ran in private mode: if it still had input the level may need more passes than were launched */
    return ( used == launched && launched > 1 ) ? used + 2 : used;
}

/* ---- a chunk's counter blocks: everything the host decides after the chunk's one synchronisation ---- */
enum { ACN_CHUNK_FITS = 0, ACN_CHUNK_OVERFLOW /* a queue overflowed: redo it smaller */, ACN_CHUNK_STACK_OVERFLOW /* the call fails */ };
typedef struct
{
    uint32_t flags;                          /* OR of the levels' QC_FLAGS, + ACN_FLAG_CHILD_OVERFLOW where a level's last pass left rays */
    int      verdict;                        /* ACN_CHUNK_* */
    uint32_t fill[ WQ_N ];                   /* high-water marks per queue */
    double   dead_share;                     /* of the marks of the deferred-shadow queue */
    /* of a chunk that fits (zero otherwise): */
    uint32_t passes_seen[ ACN_LEVEL_BLOCKS ];   /* acn_walk_passes_seen per level */
    uint64_t levels, walk_rays, walk_steps, hard_rays, shade_hit_recs, private_rays, probe_rays;
    uint32_t peak_tasks, peak_children;
} acn_chunk_report;

/* counts: `levels` blocks of QC_N words as the device left them; passes[ level ]: the launches of k_walk the level got (at most
 * ACN_MAX_WALK_PASSES); seeded: the chunk rendered the caller's rays */
static inline void acn_read_chunk( uint32_t* counts, int levels, const uint32_t* passes, int seeded, acn_chunk_report* out )
{
    memset( out, 0, sizeof( *out ) );
    /* the seeded generation of a ray call is a known demand (acn_queue_demand), not a learned one: with its word cleared the queue
     * marks, the learned passes and acn_sample_rates see the counts of a position call, where level 0 has no generation 0 */
    if( seeded ) counts[ QC_GEN + 0 ] = 0;
    for( int level = 0; level < levels; level++ )
    {
        const uint32_t* c = counts + ( size_t )level * QC_N;
        out->flags |= c[ QC_FLAGS ];
        if( c[ QC_GEN + passes[ level ] ] ) out->flags |= ACN_FLAG_CHILD_OVERFLOW;   /* rays left over by the last pass */
    }
    /* what the chunk put into each queue (high-water marks of reserved slots, dead slots included; of a chunk that
     * overflowed: at least this much): the next chunk's size and the queue capacities are derived from it.
     * How much of the marks are dead slots (the ends of the waves' reservations) is known exactly for the deferred-shadow
     * queue, whose records are counted; the share does not scale with the chunk, so a small chunk's marks over-state
     * the demand per position by 1 / ( 1 - share ) */
    uint32_t mark = 0, recs = 0;
    for( int level = 0; level < levels; level++ )
    {
        const uint32_t* c = counts + ( size_t )level * QC_N;
#define ACN_UP( q, v ) do { if( ( v ) > out->fill[ q ] ) out->fill[ q ] = ( v ); } while( 0 )
        ACN_UP( WQ_TASKS, c[ QC_TASKS ] );
        for( int k = 0; k < ACN_NCLASS; k++ ) ACN_UP( WQ_TASKS, c[ QC_CLASS0 + k ] );
        ACN_UP( WQ_CHILDREN, c[ QC_CHILDREN ] );
        ACN_UP( WQ_HARD_SHADOW, c[ QC_HARD_SHADOW ] );
        ACN_UP( WQ_HARD_PATH, c[ QC_HARD_PATH ] );
        for( int g = 0; g <= ACN_MAX_WALK_PASSES; g++ ) ACN_UP( WQ_RAYS, c[ QC_GEN + g ] );
#undef ACN_UP
        if( c[ QC_HARD_SHADOW ] > mark ) { mark = c[ QC_HARD_SHADOW ]; recs = c[ QS_HARD_SHADOW ] + c[ QS_PROBES ]; }
    }
    if( mark > 0 && recs < mark ) out->dead_share = ( double )( mark - recs ) / ( double )mark;
    /* a lost chunk first: it is redone smaller, and a stack overflow that is real shows again in the retry */
    out->verdict = out->flags & ACN_FLAGS_CHUNK_LOST ? ACN_CHUNK_OVERFLOW : out->flags & ACN_FLAG_STACK_OVERFLOW ? ACN_CHUNK_STACK_OVERFLOW : ACN_CHUNK_FITS;
    if( out->verdict != ACN_CHUNK_FITS ) return;
    for( int level = 0; level < levels; level++ )
    {
        const uint32_t* c = counts + ( size_t )level * QC_N;
        if( c[ QC_TASKS ] == 0 && c[ QS_WALK_RAYS ] == 0 ) break;
        out->levels++;
        out->walk_rays += c[ QS_WALK_RAYS ];
        out->walk_steps += c[ QS_WALK_STEPS ];
        out->hard_rays += ( uint64_t )c[ QS_HARD_SHADOW ] + c[ QS_HARD_PATH ];
        out->shade_hit_recs += c[ QS_CHILDREN ];
        if( c[ QC_TASKS ] > out->peak_tasks ) out->peak_tasks = c[ QC_TASKS ];
        if( c[ QC_CHILDREN ] > out->peak_children ) out->peak_children = c[ QC_CHILDREN ];
        out->private_rays += c[ QS_PRIVATE_RAYS ];
        out->probe_rays += c[ QS_PROBES ];
    }
    for( int level = 0; level < levels; level++ ) out->passes_seen[ level ] = acn_walk_passes_seen( counts + ( size_t )level * QC_N + QC_GEN, passes[ level ] );
}

/* ---- lanes, shards and the order of work ---- */
/* positions of lane `lane` of `lanes`: tiles lane, lane + lanes, ... of the n positions of the call */
static inline size_t acn_lane_count( size_t n, int lanes, int lane )
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
/* number of lanes for a call of n positions: the handle's ACN_LANES, fewer while a lane would get less than 32 tiles or
 * less than ~10^6 path samples' worth of work (a frame without path tracing is over before a second lane has started) */
static inline int acn_lanes_for_counts( int tun_lanes, size_t n, uint64_t path_samples )
{
    int lanes = tun_lanes;
    const size_t work = n * ( size_t )( path_samples + 1 );
    while( lanes > 1 && ( n < ( size_t )lanes * 32 * ACN_LANE_TILE || work < ( size_t )lanes << 20 ) ) lanes--;
    return lanes;
}
/* The lane plan of a handle: how many concurrent lanes a large call gets (before acn_lanes_for_counts) and the persistent grids of
 * a lane (bind_lane).  A lane is a stream, and lanes pay only while every stream has a hardware queue of its own: two lanes that
 * share a queue run their chains of ~45 launches one after the other.  HIP gives a process that asks for nothing FOUR hardware
 * queues, and the caller's stream and the handle's own are streams as well, so the default is made for that process:
 * ACN_DEFAULT_LANES lanes on ACN_DEFAULT_LANE_WGS workgroups per compute unit, k_shade too (fewer, longer chains on grids that
 * fill the chip with two of them running).  Chosen from profiles/r19/NOTES.md section 2, the run "L2 768/768/768" of its second
 * table: on four queues the 1080p frame takes 48.4 ms that way, 50.1 on two workgroups per compute unit, 52.6 on one lane, 56 - 64
 * on three or four lanes and 60.6 on the six of round 4.  A host that exports more queues (GPU_MAX_HW_QUEUES=8) sets ACN_LANES:
 * a given count is the host's, on the round-4 grids -- one workgroup per compute unit, k_shade one and a half -- that six lanes
 * with a queue each were measured on (profiles/r04/ab_lanes6_*).  Nothing here reads the process: the arguments are the handle's
 * tunables (lanes_given: ACN_LANES was set, lanes_env its value; *_grid_env: ACN_GRID / ACN_SHADE_GRID / ACN_WALK_GRID, 0 = not
 * set) and the compute units of its device. */
#define ACN_DEFAULT_LANES 2
#define ACN_DEFAULT_LANE_WGS 3
#define ACN_MAX_LANES 16
typedef struct { int lanes; unsigned grid, shade_grid, walk_grid; } acn_lane_plan_t;
static inline acn_lane_plan_t acn_lane_plan( int lanes_given, int lanes_env, unsigned cus, unsigned grid_env, unsigned shade_grid_env, unsigned walk_grid_env )
{
    acn_lane_plan_t p;
    p.lanes = lanes_given ? ( lanes_env < 1 ? 1 : lanes_env > ACN_MAX_LANES ? ACN_MAX_LANES : lanes_env ) : ACN_DEFAULT_LANES;
    p.grid = grid_env ? grid_env : lanes_given ? cus : cus * ACN_DEFAULT_LANE_WGS;
    p.shade_grid = shade_grid_env ? shade_grid_env : lanes_given ? cus * 3u / 2u : cus * ACN_DEFAULT_LANE_WGS;
    p.walk_grid = walk_grid_env ? walk_grid_env : p.grid;
    return p;
}

/* 1: the call's queues cannot hold it in one chunk per lane within the workspace bound, it runs on one lane (render_dispatch).
 * was_one_lane: sticky by 30 % -- rates move a little from call to call, and changing the arrangement re-allocates everything */
static inline int acn_one_lane( const double* rate, int seeded, size_t n, const size_t* rec_bytes, size_t budget, int was_one_lane )
{
    double need = 0;
    for( int q = 0; q < WQ_N; q++ ) need += acn_queue_demand( rate, q, seeded ) * ( double )n / 0.7 * ( double )rec_bytes[ q ];
    return need > ( was_one_lane ? 0.7 : 1.0 ) * ( double )budget;
}
/* the order of work: tiles of 1 << shift positions in a multiplicative stride over the call (TileOrder).  Returns the tiles;
 * *mul is coprime to them */
static inline uint32_t acn_tile_order( size_t n, int shift, uint32_t* mul )
{
    const uint32_t n_tiles = ( uint32_t )( ( n + ( ( 1u << shift ) - 1 ) ) >> shift );
    *mul = 1;
    if( n_tiles > 2 )
    {
        uint64_t m = ( uint64_t )( 0.6180339887 * n_tiles ) | 1u;
        for( ;; )
        {
            uint64_t a = m, b = n_tiles;
            while( b ) { uint64_t t = a % b; a = b; b = t; }
            if( a == 1 ) break;
            m += 2;
        }
        *mul = ( uint32_t )( m % n_tiles );
    }
    return n_tiles;
}

#endif /* ACN_QUEUEPLAN_H */
