/* acn_stage_host.h -- what acn_stage_plan / acn_run_stage (include/actinon_hip.h, the stage-runner test seam) do without the GPU: every
 * argument check, and the capacities of the output queues.  Plain C++, no HIP header: k_stage.hip calls acn_stage_check before it
 * launches anything, and tests/csrc/stage_cpu.cpp compiles the header on its own into a program that runs under the address and
 * undefined-behaviour sanitizers (tests/csrc/stage_walk_cpu.cpp: the walk's checks, acn_stage_walk_check).  The five input records
 * are restated here as plain structs; k_stage.hip asserts that they are the pipeline's (sizes and offsets). */
#ifndef ACN_STAGE_HOST_H
#define ACN_STAGE_HOST_H

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>

#include "actinon_hip.h"
#include "acn_counts.h"

struct acn_stage_v3 { double x, y, z; };
/* HitRec of acn_records.h */
struct acn_stage_hitrec
{
    acn_stage_v3 p, d; double offs; acn_stage_v3 exit_nor, T; double intensity;
    int32_t exit_obj, enter_obj, depth; uint32_t pixel;
};
/* DTask of acn_records.h */
struct acn_stage_dtask
{
    acn_stage_v3 pos, surface_d, ray_projection; double theta_i, on_a, on_b, diffuse_intensity; acn_stage_v3 Tc;
    uint64_t rv; int32_t depth; uint32_t pixel;
};

/* HardShadow and HardPath of acn_records.h */
struct acn_stage_hardshadow { acn_stage_v3 pos, d; double limit; acn_stage_v3 contrib; uint32_t pixel, pad; };
struct acn_stage_hardpath { acn_stage_v3 pos, d, T; double intensity; int32_t depth; uint32_t pixel, resume, pad; };
/* RayTask of acn_records.h */
struct acn_stage_raytask { acn_stage_v3 p, d, T; double intensity; int32_t depth; uint32_t pixel; };

/* what the checks read of the uploaded scene */
struct acn_stage_scene
{
    uint32_t n_nodes, n_lights;
    uint64_t direct_samples, path_samples;
    double trace_min_intensity;
};

#define ACN_STAGE_DEAD 0xFFFFFFFFu
#define ACN_STAGE_MAX_GRID 64u          /* workgroups of a stage launch: 256 waves at most */
#define ACN_STAGE_MAX_CAP ( 1u << 26 )  /* records of one output queue */

/* samples of a loop as shade_hit and k_shade count them: ( uint64_t )( samples * diffuse_intensity ), at least 1.  *ok: the product is
 * finite, not negative and within ACN_STAGE_MAX_SAMPLES (so the conversion is defined) */
static inline uint64_t acn_stage_samples( uint64_t samples, double diffuse_intensity, bool* ok )
{
    const double v = ( double )samples * diffuse_intensity;
    if( !( v >= 0.0 ) || !( v < ( double )ACN_STAGE_MAX_SAMPLES + 1.0 ) ) { *ok = false; return 0; }
    const uint64_t n = ( uint64_t )v;
    return n == 0 ? 1 : n;
}

static inline bool acn_stage_finite_ray( const acn_stage_v3& p, const acn_stage_v3& d )
{
    return std::isfinite( p.x ) && std::isfinite( p.y ) && std::isfinite( p.z ) && std::isfinite( d.x ) && std::isfinite( d.y ) && std::isfinite( d.z );
}
#define ACN_STAGE_RESUME_FLAG 2u        /* ACN_RESUME_FLAG of acn_device.h: the word is a resume word */

/* slots a wave reserves at a time: ACN_QCHUNK of k_shade, chunks_resize( n ) of k_shade_hits (acn_queues.h) */
static inline uint32_t acn_stage_chunk( uint32_t stage, uint32_t n, uint32_t grid )
{
    if( stage != ACN_STAGE_SHADE_HITS ) return 64u;
    uint32_t size = ( ( n / ( grid * 4u ) ) / 8u ) & ~63u;
    return size < 64u ? 64u : size > 512u ? 512u : size;
}

/* every check of a stage call, then the capacities: the records the input can produce at most plus one reservation per wave (a wave
 * leaves the unused end of at most one reservation per queue behind).  have_handle: the caller holds one. */
static inline int acn_stage_check( bool have_handle, const acn_stage_args* a, const acn_stage_scene& sc, acn_stage_caps* caps, std::string* msg )
{
    if( !have_handle ) { *msg = "null argument: handle"; return ACN_ERR_ARG; }
    if( !a || !caps ) { *msg = "null argument: acn_stage_args / acn_stage_caps"; return ACN_ERR_ARG; }
    if( a->stage >= ACN_STAGE_N ) { *msg = "unknown stage " + std::to_string( a->stage ); return ACN_ERR_ARG; }
    if( a->flags & ~( ACN_STAGE_NO_PRUNE | ACN_STAGE_NO_LEAF_LIGHTS | ACN_STAGE_NO_EMIT_TERMS | ACN_STAGE_COUNT_WORK ) ) { *msg = "unknown acn_stage_args.flags bits"; return ACN_ERR_ARG; }
    if( !a->in ) { *msg = "null argument: in"; return ACN_ERR_ARG; }
    if( a->n == 0 || a->n > ACN_STAGE_MAX_RECORDS ) { *msg = "n " + std::to_string( a->n ) + " is outside 1 .. 2^20 records"; return ACN_ERR_ARG; }
    const bool shade = a->stage == ACN_STAGE_SHADE;
    const bool hard = a->stage == ACN_STAGE_HARD_SHADOW || a->stage == ACN_STAGE_HARD_PATH;
    uint64_t sum_direct = 0, sum_path = 0;
    if( hard )
    {
        if( a->cls > ACN_STAGE_MAX_GRID ) { *msg = "workgroups (cls) " + std::to_string( a->cls ) + " are above 64"; return ACN_ERR_ARG; }
        for( uint32_t i = 0; i < a->n; i++ )
        {
            const std::string who = ( a->stage == ACN_STAGE_HARD_SHADOW ? "hard-shadow record " : "hard-path record " ) + std::to_string( i );
            const acn_stage_hardshadow* hs = a->stage == ACN_STAGE_HARD_SHADOW ? ( const acn_stage_hardshadow* )a->in + i : nullptr;
            const acn_stage_hardpath* hp = hs ? nullptr : ( const acn_stage_hardpath* )a->in + i;
            const uint32_t pixel = hs ? hs->pixel : hp->pixel;
            if( pixel == ACN_STAGE_DEAD ) continue;
            if( pixel >= a->n ) { *msg = who + ": pixel " + std::to_string( pixel ) + " is not below n"; return ACN_ERR_ARG; }
            if( !acn_stage_finite_ray( hs ? hs->pos : hp->pos, hs ? hs->d : hp->d ) ) { *msg = who + ": the ray is not finite"; return ACN_ERR_ARG; }
            if( hs && !( hs->limit > 0.0 ) ) { *msg = who + ": limit is not above 0"; return ACN_ERR_ARG; }
            const uint32_t word = hs ? hs->pad : hp->resume;
            if( ( word & 1u ) && ( ( word & ACN_STAGE_RESUME_FLAG ) || hp ) ) { *msg = who + ": bit 0 of the word is set beside a resume word"; return ACN_ERR_ARG; }
            if( !( word & ACN_STAGE_RESUME_FLAG ) && word > 1u ) { *msg = who + ": a word without the resume flag names candidates"; return ACN_ERR_ARG; }
            if( hp && ( hp->depth < 0 || hp->depth > ACN_STAGE_MAX_DEPTH ) ) { *msg = who + ": depth " + std::to_string( hp->depth ) + " is outside 0 .. 2^20"; return ACN_ERR_ARG; }
        }
    }
    else if( !shade )
    {
        const acn_stage_hitrec* r = ( const acn_stage_hitrec* )a->in;
        for( uint32_t i = 0; i < a->n; i++ )
        {
            const std::string who = "hit record " + std::to_string( i );
            if( r[ i ].pixel == ACN_STAGE_DEAD ) continue;
            if( r[ i ].pixel >= a->n ) { *msg = who + ": pixel " + std::to_string( r[ i ].pixel ) + " is not below n"; return ACN_ERR_ARG; }
            if( r[ i ].depth < 0 || r[ i ].depth > ACN_STAGE_MAX_DEPTH ) { *msg = who + ": depth " + std::to_string( r[ i ].depth ) + " is outside 0 .. 2^20"; return ACN_ERR_ARG; }
            for( int32_t o : { r[ i ].exit_obj, r[ i ].enter_obj } )
                if( o < -1 || ( o >= 0 && ( uint32_t )o >= sc.n_nodes ) ) { *msg = who + ": object " + std::to_string( o ) + " is no node of the scene"; return ACN_ERR_ARG; }
        }
    }
    else
    {
        if( a->cls > 3 ) { *msg = "size class " + std::to_string( a->cls ) + " is above 3"; return ACN_ERR_ARG; }
        const uint32_t world = a->shard_world ? a->shard_world : 1u;
        if( a->shard_rank >= world ) { *msg = "shard_rank " + std::to_string( a->shard_rank ) + " is not below shard_world"; return ACN_ERR_ARG; }
        if( !a->index ) { *msg = "null argument: index"; return ACN_ERR_ARG; }
        if( a->n_index == 0 || a->n_index > ACN_STAGE_MAX_RECORDS ) { *msg = "n_index " + std::to_string( a->n_index ) + " is outside 1 .. 2^20 entries"; return ACN_ERR_ARG; }
        const acn_stage_dtask* t = ( const acn_stage_dtask* )a->in;
        for( uint32_t k = 0; k < a->n_index; k++ )
        {
            const uint32_t i = a->index[ k ];
            if( i == ACN_STAGE_DEAD ) continue;
            if( i >= a->n ) { *msg = "index entry " + std::to_string( k ) + ": task " + std::to_string( i ) + " is not below n"; return ACN_ERR_ARG; }
            const std::string who = "task " + std::to_string( i );
            if( t[ i ].pixel >= a->n ) { *msg = who + ": pixel " + std::to_string( t[ i ].pixel ) + " is not below n"; return ACN_ERR_ARG; }
            if( t[ i ].depth < 0 || t[ i ].depth > ACN_STAGE_MAX_DEPTH ) { *msg = who + ": depth " + std::to_string( t[ i ].depth ) + " is outside 0 .. 2^20"; return ACN_ERR_ARG; }
            bool ok = true;
            const uint64_t nd = sc.n_lights ? acn_stage_samples( sc.direct_samples, t[ i ].diffuse_intensity, &ok ) : 0;
            const uint64_t np = sc.path_samples && t[ i ].depth > 10 ? acn_stage_samples( sc.path_samples, t[ i ].diffuse_intensity, &ok ) : 0;
            if( !ok ) { *msg = who + ": diffuse_intensity asks for a sample count that is not within 0 .. 2^16"; return ACN_ERR_ARG; }
            sum_direct += nd * sc.n_lights;
            sum_path += np;
        }
    }
    acn_stage_caps c;
    memset( &c, 0, sizeof( c ) );
    const uint32_t items = shade ? a->n_index : a->n;
    c.grid = hard ? ( a->cls ? a->cls : ( items + 255u ) / 256u ) : ( items + 3u ) / 4u;
    c.grid = c.grid > ACN_STAGE_MAX_GRID ? ACN_STAGE_MAX_GRID : c.grid;
    c.chunk = acn_stage_chunk( a->stage, a->n, c.grid );
    const uint64_t slack = ( uint64_t )c.grid * 4u * c.chunk;
    uint64_t tasks, rays, children, hs, hp;
    if( shade ) { tasks = a->n_index; rays = 0; children = sum_path + slack; hp = sum_path + slack; hs = sum_direct + sum_path + slack; }
    else if( a->stage == ACN_STAGE_HARD_SHADOW ) { tasks = 0; rays = 0; children = 0; hp = 0; hs = a->n; }                      /* the input queue; nothing is appended */
    else if( a->stage == ACN_STAGE_HARD_PATH )   { tasks = 0; rays = 0; children = ( uint64_t )a->n + slack; hp = a->n; hs = 0; }   /* a hit record per ray at most */
    else        { tasks = ( uint64_t )a->n + slack; rays = 3ull * a->n + slack; children = a->n; hp = 0; hs = 3ull * a->n + slack; }
    for( uint64_t v : { tasks, rays, children, hs, hp } )
        if( v > ACN_STAGE_MAX_CAP ) { *msg = "the input can produce " + std::to_string( v ) + " records of one queue: above 2^26"; return ACN_ERR_ARG; }
    c.cap_tasks = ( uint32_t )tasks; c.cap_rays = ( uint32_t )rays; c.cap_children = ( uint32_t )children;
    c.cap_hard_shadow = ( uint32_t )hs; c.cap_hard_path = ( uint32_t )hp;
    *caps = c;
    return ACN_OK;
}

/* ---- the walk (acn_stage_walk_plan / acn_run_stage_walk) ---- */

/* input slots of a walk call: the rays, or every slot of the tiles of 256 positions of the camera form (ACN_ORDER_SHIFT) */
static inline uint32_t acn_stage_walk_slots( const acn_stage_walk_args* a ) { return a->camera ? ( ( a->n + 255u ) >> 8 ) << 8 : a->n; }

/* every check of a walk call, then the launch and the capacities.  Each launch of k_walk appends to the tasks, to the probes and
 * to ONE ray buffer (the next generation's, which it fills from slot 0), so the slack of a wave's reservations is one per launch
 * for the tasks and the probes and one for a ray buffer. */
static inline int acn_stage_walk_check( bool have_handle, const acn_stage_walk_args* a, const acn_stage_scene& sc, acn_stage_caps* caps, std::string* msg )
{
    if( !have_handle ) { *msg = "null argument: handle"; return ACN_ERR_ARG; }
    if( !a || !caps ) { *msg = "null argument: acn_stage_walk_args / acn_stage_caps"; return ACN_ERR_ARG; }
    if( a->stage != ACN_STAGE_WALK ) { *msg = "stage " + std::to_string( a->stage ) + " is not ACN_STAGE_WALK"; return ACN_ERR_ARG; }
    if( a->flags & ~( ACN_STAGE_NO_PRUNE | ACN_STAGE_NO_EMIT_TERMS | ACN_STAGE_GLOBAL_NODES | ACN_STAGE_COUNT_WORK ) ) { *msg = "unknown acn_stage_walk_args.flags bits"; return ACN_ERR_ARG; }
    if( a->camera ? a->in != nullptr : a->pos_xy != nullptr ) { *msg = "both input forms: rays and the camera form"; return ACN_ERR_ARG; }
    if( !a->camera && !a->in ) { *msg = "neither input form: null argument in without the camera form"; return ACN_ERR_ARG; }
    if( a->n == 0 || a->n > ACN_STAGE_MAX_RECORDS ) { *msg = "n " + std::to_string( a->n ) + " is outside 1 .. 2^20 records"; return ACN_ERR_ARG; }
    if( a->passes == 0 || a->passes > ACN_MAX_WALK_PASSES ) { *msg = "passes " + std::to_string( a->passes ) + " are outside 1 .. 32"; return ACN_ERR_ARG; }
    if( a->stack_cap == 0 || a->stack_cap > ACN_STAGE_WALK_MAX_STACK ) { *msg = "stack_cap " + std::to_string( a->stack_cap ) + " is outside 1 .. 4096"; return ACN_ERR_ARG; }
    if( a->stack_use > a->stack_cap ) { *msg = "stack_use " + std::to_string( a->stack_use ) + " is above stack_cap"; return ACN_ERR_ARG; }
    if( a->fetch < 64u || a->fetch > ACN_STAGE_MAX_RECORDS ) { *msg = "fetch " + std::to_string( a->fetch ) + " is outside 64 .. 2^20"; return ACN_ERR_ARG; }
    if( a->grid > ACN_STAGE_MAX_GRID ) { *msg = "workgroups (grid) " + std::to_string( a->grid ) + " are above 64"; return ACN_ERR_ARG; }
    if( a->room_rays < a->n ) { *msg = "room_rays " + std::to_string( a->room_rays ) + " is below n"; return ACN_ERR_ARG; }
    if( !a->camera )
    {
        const acn_stage_raytask* r = ( const acn_stage_raytask* )a->in;
        for( uint32_t i = 0; i < a->n; i++ )
        {
            const std::string who = "ray " + std::to_string( i );
            if( r[ i ].pixel == ACN_STAGE_DEAD ) continue;
            if( r[ i ].pixel >= a->n ) { *msg = who + ": pixel " + std::to_string( r[ i ].pixel ) + " is not below n"; return ACN_ERR_ARG; }
            if( !acn_stage_finite_ray( r[ i ].p, r[ i ].d ) ) { *msg = who + ": the ray is not finite"; return ACN_ERR_ARG; }
            if( !( std::isfinite( r[ i ].T.x ) && std::isfinite( r[ i ].T.y ) && std::isfinite( r[ i ].T.z ) ) ) { *msg = who + ": T is not finite"; return ACN_ERR_ARG; }
            if( r[ i ].d.x == 0.0 && r[ i ].d.y == 0.0 && r[ i ].d.z == 0.0 ) { *msg = who + ": the direction has no length"; return ACN_ERR_ARG; }
            if( r[ i ].depth < 1 || r[ i ].depth > ACN_STAGE_MAX_DEPTH ) { *msg = who + ": depth " + std::to_string( r[ i ].depth ) + " is outside 1 .. 2^20"; return ACN_ERR_ARG; }
            /* (a NaN intensity fails the first test) */
            if( !std::isfinite( r[ i ].intensity ) || r[ i ].intensity < sc.trace_min_intensity )
            { *msg = who + ": the intensity is not finite or below trace_min_intensity (such a ray is a probe, never a queued ray)"; return ACN_ERR_ARG; }
        }
    }
    acn_stage_caps c;
    memset( &c, 0, sizeof( c ) );
    c.grid = a->grid ? a->grid : ( acn_stage_walk_slots( a ) + 255u ) / 256u;
    c.grid = c.grid > ACN_STAGE_MAX_GRID ? ACN_STAGE_MAX_GRID : c.grid;
    c.chunk = ACN_QCHUNK;
    const uint64_t slack = ( uint64_t )c.grid * 4u * c.chunk;
    const uint64_t rays = ( uint64_t )a->room_rays + slack, tasks = ( uint64_t )a->room_rays + slack * a->passes, hs = 3ull * a->room_rays + slack * a->passes;
    for( uint64_t v : { tasks, rays, hs } )
        if( v > ACN_STAGE_MAX_CAP ) { *msg = "room_rays asks for " + std::to_string( v ) + " records of one queue: above 2^26"; return ACN_ERR_ARG; }
    c.cap_tasks = ( uint32_t )tasks; c.cap_rays = ( uint32_t )rays; c.cap_hard_shadow = ( uint32_t )hs;
    *caps = c;
    return ACN_OK;
}

#endif
