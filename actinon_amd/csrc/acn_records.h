/* acn_records.h -- the records the pipeline kernels hand each other, the order of work and the fixed-point pixel sum: what acn_launch.h,
 * the host units and the side kernels need of the pipeline (the kernels: acn_queues.h and acn_k_walk.h, acn_k_shade.h, acn_k_hard.h). */
#ifndef ACN_RECORDS_H
#define ACN_RECORDS_H

#include "acn_dev_base.h"    /* V3, DEV, f_abs */
#include "acn_dev_scene.h"   /* DevScene for acn_launch.h (and through it acn_counts.h: the ACN_FLAG_* bits); no ray layer */

/* ---- fixed-point pixel accumulation ---- */
#define ACN_FIX_SCALE 1099511627776.0          /* 2^40 */
#define ACN_FIX_INV   9.094947017729282e-13    /* 2^-40 */
#define ACN_FIX_CLAMP 16384.0

DEV long long to_fixed( double x )
{
    x = x < ACN_FIX_CLAMP ? x : ACN_FIX_CLAMP;
    x = x > -ACN_FIX_CLAMP ? x : -ACN_FIX_CLAMP;   /* NaN falls through both and converts to 0 below */
    if( x != x ) return 0;
    return __double2ll_rn( x * ACN_FIX_SCALE );
}

/* `flags`: the device word for ACN_FLAG_* bits; a clamped contribution is reported, not an error */
DEV void pixel_add( unsigned long long* accum, uint32_t* flags, size_t i, V3 c )
{
    long long x = to_fixed( c.x ), y = to_fixed( c.y ), z = to_fixed( c.z );
    if( f_abs( c.x ) > ACN_FIX_CLAMP || f_abs( c.y ) > ACN_FIX_CLAMP || f_abs( c.z ) > ACN_FIX_CLAMP ) atomicOr( flags, ACN_FLAG_CLAMPED );
    if( x ) atomicAdd( &accum[ i * 3 + 0 ], ( unsigned long long )x );
    if( y ) atomicAdd( &accum[ i * 3 + 1 ], ( unsigned long long )y );
    if( z ) atomicAdd( &accum[ i * 3 + 2 ], ( unsigned long long )z );
}

/* ---- records ---- */

/* pending ray of the specular walk */
struct RayTask
{
    V3 p, d;
    V3 T;               /* colour throughput applied to whatever this ray returns */
    double intensity;
    int depth;
    uint32_t pixel;     /* ACN_INVALID: dead slot */
};

/* a diffuse shading point whose sample loops are still to run (scene.c:526-621) */
struct DTask
{
    V3 pos;              /* surface.p */
    V3 surface_d;        /* -exit_nor */
    V3 ray_projection;
    double theta_i, on_a, on_b;
    double diffuse_intensity;
    V3 Tc;               /* T * obj_color( enter_obj ) */
    uint64_t rv;         /* seed of the shading point's LCG stream (scene.c:537) */
    int depth;
    uint32_t pixel;
};

/* a path-sample hit: the arguments of the recursive scene_s_lum call of scene.c:610 */
struct HitRec
{
    V3 p, d;
    double offs;
    V3 exit_nor;
    V3 T;
    double intensity;
    int exit_obj, enter_obj;
    int depth;
    uint32_t pixel;      /* ACN_INVALID: dead slot */
};

/* a shadow ray of k_shade that entered the envelope of a CSG / SDF / compound element: finished by k_hard_shadow */
struct HardShadow
{
    V3 pos, d;
    double limit;        /* distance of the light hit */
    V3 contrib;          /* what the sample adds to the pixel if it is not occluded */
    uint32_t pixel, pad; /* pixel == ACN_INVALID: dead slot.  pad bit 0: a probe of a specular ray (see probe_push): the light root counts too;
                            bits 1 .. 31: the resume word of k_shade's in-line pass over the matter root (acn_dev_traverse.h: ACN_RESUME_FLAG,
                            resume_record); bit 1 clear: nothing is known, every element is to be tested */
};

/* a path ray of k_shade that did: k_hard_path finishes the transition hit */
struct HardPath
{
    V3 pos, d;
    V3 T;
    double intensity;
    int depth;
    uint32_t pixel;      /* ACN_INVALID: dead slot */
    uint32_t resume;     /* bits 1 .. 31: the resume word, as in HardShadow.pad (depth has no bound, so the word has a field of its own) */
    uint32_t pad;
};
static_assert( sizeof( HardShadow ) == 88 && sizeof( HardPath ) == 96, "record sizes: DESIGN.md section 3" );

#define ACN_INVALID 0xFFFFFFFFu
#define ACN_INVALID_SLOT 0xFFFFFFFFu
/* (the counter block of a path level -- QC_*, QS_*, ACN_NCLASS, ACN_MAX_WALK_PASSES, ACN_QCHUNK -- and the ACN_FLAG_* bits: acn_counts.h) */

/* how many lanes of `mask` lie below the calling lane: two VALU instructions, no lane index or lane mask kept in registers */
DEV uint32_t lanes_below( unsigned long long mask )
{
    return __builtin_amdgcn_mbcnt_hi( ( uint32_t )( mask >> 32 ), __builtin_amdgcn_mbcnt_lo( ( uint32_t )mask, 0u ) );
}

/* The order in which the sample positions of a call are worked off.  A chunk is a contiguous range of SLOTS; slot s
 * stands for position  tile( s / 256 ) * 256 + s % 256  with  tile( t ) = t * mul mod n_tiles  (mul coprime to n_tiles:
 * a bijection).  Tiles of 256 consecutive positions keep neighbouring pixels in one workgroup; the multiplicative stride
 * spreads the tiles of any chunk over the whole frame, so that every chunk of a call sees the same mix of sky, floor
 * and glass -- the queue fill of one chunk then predicts the next one's (launch_render sizes chunks that way). */
#define ACN_ORDER_SHIFT 8   /* tiles of 256 positions: the four waves of a workgroup work on neighbouring pixels and visit the same nodes
                               (tiles of 64 mix a small chunk better, but hanging_lamp 2160p p1024 -- 550 KB of nodes -- ran 25 % slower
                               and the small scenes 1 - 3 %) */
struct TileOrder
{
    uint32_t n;         /* positions of the call */
    uint32_t n_tiles;   /* ceil( n / 256 ) */
    uint32_t mul;
    uint32_t sample_stride;   /* > 0: the learning pass of a cold handle (learn_rates): slot s stands for position s * sample_stride */
    DEV uint32_t position( uint32_t slot ) const
    {
        if( sample_stride ) { const uint64_t p = ( uint64_t )slot * sample_stride; return p < n ? ( uint32_t )p : 0xFFFFFFFFu; }
        uint32_t tile = ( uint32_t )( ( ( uint64_t )( slot >> ACN_ORDER_SHIFT ) * mul ) % n_tiles );
        return ( tile << ACN_ORDER_SHIFT ) + ( slot & ( ( 1u << ACN_ORDER_SHIFT ) - 1u ) );
    }
};
#endif /* ACN_RECORDS_H */
