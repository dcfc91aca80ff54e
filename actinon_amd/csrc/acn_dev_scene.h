/* acn_dev_scene.h -- the device-resident scene and what every kernel has beside it: the dynamic LDS array, DevSceneT and its views,
 * the work counters, the phase timers of the diagnostic builds and the by-value scene reference of the real calls. */
#ifndef ACN_DEV_SCENE_H
#define ACN_DEV_SCENE_H

#include "acn_dev_base.h"
#include "acn_counts.h"   /* the ACN_FLAG_* bits of a chunk's flag word */

#pragma clang fp contract(off)

/* dynamic LDS of the machine kernels: [ staged node array (optional) ][ CSG stacks of the block's 256 lanes ] */
extern __shared__ __attribute__( ( aligned( 16 ) ) ) double acn_lds_raw[];
/* the stacks ( ACN_LDS_STACK_BYTES ) and behind them the parked ray origins ( ACN_LDS_ORG_BYTES ): acn_tables.h */
#define ACN_NO_LDS_STACK 0xFFFFFFFFu

/* device-resident scene, parameterised by where the node array is read from */
template< class NP >
struct DevSceneT
{
    NP nodes;
    const GNode ACN_CONST* gnodes;   /* the node array in global memory, whatever `nodes` points to (wave-uniform reads: scalar loads) */
    MatP  mats;
    ElemP elems;
    TexP  textures;
    int32_t light_root, matter_root;
    uint32_t n_nodes, n_elems;
    acn_params prm;
    /* camera basis, computed on the device by k_camera_setup with the same expressions as the oracle */
    M3 camera_rotation;
    double unit_f;
    uint32_t* flags;     /* device word for ACN_FLAG_* error bits */
    uint32_t lds_stack;  /* byte offset of the CSG stack area in dynamic LDS, ACN_NO_LDS_STACK if the kernel has none */
    uint32_t prune_base; /* elems[ prune_base + node ]: offset of the node's prune program in elems[], or -1 */
    uint32_t class0_min; /* shading tasks with more samples than this run on 64 lanes (ACN_CLASS0_MIN, acn_queues.h: size_class) */
    const SCEntry* sc_table;   /* pre-order tables of the simple compounds */
    const double* sc_spheres;  /* ( pos, radius ) of the sphere leaves of those tables, see SCEntry.flags */
    static constexpr bool prune = false;
    static constexpr bool park = false;   /* the lock-step machines keep the ray origin in LDS (OrgLds): only where the kernel owns the slot */
};
/* the same scene for the "extras" kernel variants: interval-prune programs and in-line simple compounds.  Launched
 * only when the upload step produced either, so that the kernels of plain scenes (wine_glass) do not carry their code */
template< class NP > struct DevScenePT : DevSceneT< NP > { static constexpr bool prune = true; };
template< class BASE > struct ParkedScene : BASE { static constexpr bool park = true; };
typedef DevSceneT< NodeP > DevScene;

/* the same scene with its node array read from another address space */
template< class NP2 >
__device__ __forceinline__ DevSceneT< NP2 > scene_rebind( const DevScene& sc, NP2 nodes )
{
    DevSceneT< NP2 > r;
    r.nodes = nodes; r.gnodes = sc.nodes; r.mats = sc.mats; r.elems = sc.elems; r.textures = sc.textures;
    r.light_root = sc.light_root; r.matter_root = sc.matter_root; r.n_nodes = sc.n_nodes; r.n_elems = sc.n_elems;
    r.prm = sc.prm; r.camera_rotation = sc.camera_rotation; r.unit_f = sc.unit_f; r.flags = sc.flags; r.lds_stack = sc.lds_stack; r.prune_base = sc.prune_base; r.class0_min = sc.class0_min; r.sc_table = sc.sc_table; r.sc_spheres = sc.sc_spheres;
    return r;
}

template< bool PR, bool PK = false, class NP2 >
__device__ __forceinline__ auto scene_view( const DevScene& sc, NP2 nodes )
{
    if constexpr( PR )
    {
        if constexpr( PK ) { ParkedScene< DevScenePT< NP2 > > r; static_cast< DevSceneT< NP2 >& >( r ) = scene_rebind( sc, nodes ); return r; }
        else               { DevScenePT< NP2 > r; static_cast< DevSceneT< NP2 >& >( r ) = scene_rebind( sc, nodes ); return r; }
    }
    else
    {
        if constexpr( PK ) { ParkedScene< DevSceneT< NP2 > > r; static_cast< DevSceneT< NP2 >& >( r ) = scene_rebind( sc, nodes ); return r; }
        else return scene_rebind( sc, nodes );
    }
}

/* the scene as a machine kernel sees it: the node array where that kernel reads it (LDS: staged there by ACN_STAGE_NODES) */
template< bool PR, bool LDS > __device__ __forceinline__ auto machine_view( const DevScene& sc )
{
    if constexpr( LDS ) return scene_view< PR, true >( sc, ( LdsNodeP )acn_lds_raw );
    else                return scene_view< PR, true >( sc, sc.nodes );
}

enum
{
    CNT_TRANS_RAY = 0, CNT_SHADOW_RAY, CNT_OBJ_HIT, CNT_LUM, CNT_CAP_SAMPLE, CNT_SIDE, CNT_SDF_EVAL, CNT_OVERFLOW, CNT_N
};

/* per-lane event counts of one launch (32 bit each), wave-reduced into 64-bit global counters at kernel end.
 * Cnt< false > compiles to nothing: the counting kernels are only used when ACN_OPT_COUNT_WORK is set. */
template< bool ON > struct Cnt;
template<> struct Cnt< true >
{
    static constexpr bool counting = true;
    unsigned c[ CNT_N ];
    unsigned long long flop;   /* sum of event costs, acn_costs.h */
    unsigned transc;           /* transcendental calls */
    __device__ __forceinline__ void clear() { for( int k = 0; k < CNT_N; k++ ) c[ k ] = 0; flop = 0; transc = 0; }
    __device__ __forceinline__ void inc( int k ) { c[ k ]++; }
    __device__ __forceinline__ void add( int k, unsigned v ) { c[ k ] += v; }
    __device__ __forceinline__ void cost( unsigned f, unsigned t = 0 ) { flop += f; transc += t; }
};
template<> struct Cnt< false >
{
    static constexpr bool counting = false;
    __device__ __forceinline__ void clear() {}
    __device__ __forceinline__ void inc( int ) {}
    __device__ __forceinline__ void add( int, unsigned ) {}
    __device__ __forceinline__ void cost( unsigned, unsigned = 0 ) {}
};
/* the leaf routines (acn_dev_leaves.h) take the lane's counters as their last argument, written out at every call site
 * (our own pruning tests, which are not events of the reference's algorithm, pass ACN_NO_CNT) */
#define ACN_NO_CNT ( ( Cnt< false >* )nullptr )

/* Phase timers (diagnostic builds only: make ... EXTRA=-DACN_PHASE_TIMERS).  Every wave keeps a time stamp and ACN_PH_N
 * accumulators in LDS; ACN_LAP( k ) books the shader-clock time since the wave's previous mark on phase k, whichever
 * lanes are active.  phase_flush adds the wave's sums to counters[ CNT_N + 2 + 16 * kernel + k ] at kernel end. */
#define ACN_PH_N 16
#define ACN_PH_KERNELS 4
#define ACN_CNT_SLOTS ( CNT_N + 2 + ACN_PH_N * ACN_PH_KERNELS )
enum { PH_OTHER = 0, PH_LIGHT, PH_ROOT_LEAF, PH_PRUNE, PH_M_LEAF, PH_M_PAIR, PH_M_FRAME, PH_M_SIDE, PH_SHADE, PH_COMPOUND, PH_FETCH, PH_TAIL,
       /* k_shade alone (its slots 0 .. 3 hold the round tallies of ACN_TALLY; slots 12 .. 15 are the machine tallies of the other
        * kernels, acn_unimachine.h).  All 16 slots are taken, so these two are clean only where k_shade enters no machine: in the
        * LEAF_LIGHTS variants.  With a light that is no leaf, light_hit_call's machine adds its lanes and entries (counts, not
        * ticks) into them: read the set-up shares of such a scene with that in mind */
       PH_LIGHT_SETUP, PH_PATH_SETUP };
#ifdef ACN_PHASE_TIMERS
__shared__ unsigned long long acn_phase_lds[ 4 ][ ACN_PH_N + 1 ];
__device__ __forceinline__ void phase_lap( int k )
{
    unsigned long long now = __builtin_readcyclecounter();
    unsigned long long ex = __ballot( 1 );
    if( ( int )( threadIdx.x & 63 ) == __ffsll( ( long long )ex ) - 1 )
    {
        unsigned long long* w = acn_phase_lds[ threadIdx.x >> 6 ];
        w[ 1 + k ] += now - w[ 0 ];
        w[ 0 ] = now;
    }
}
__device__ __forceinline__ void phase_init()
{
    if( ( threadIdx.x & 63 ) == 0 )
    {
        unsigned long long* w = acn_phase_lds[ threadIdx.x >> 6 ];
        for( int k = 1; k <= ACN_PH_N; k++ ) w[ k ] = 0;
        w[ 0 ] = __builtin_readcyclecounter();
    }
}
__device__ __forceinline__ void phase_flush( unsigned long long* counters, int kernel )
{
    if( ( threadIdx.x & 63 ) == 0 )
    {
        unsigned long long* w = acn_phase_lds[ threadIdx.x >> 6 ];
        for( int k = 0; k < ACN_PH_N; k++ ) if( w[ 1 + k ] ) atomicAdd( &counters[ CNT_N + 2 + ACN_PH_N * kernel + k ], w[ 1 + k ] );
    }
}
/* diagnostic tallies in the same slots: [ 12 ] lanes that entered a lock-step machine, [ 13 ] machine entries (waves),
 * [ 14 ] lanes active at leaf evaluations inside it, [ 15 ] leaf evaluations */
__device__ __forceinline__ void phase_tally( int k, bool x )
{
    unsigned long long ex = __ballot( 1 ), m = __ballot( x );
    if( ( int )( threadIdx.x & 63 ) == __ffsll( ( long long )ex ) - 1 )
    {
        unsigned long long* w = acn_phase_lds[ threadIdx.x >> 6 ];
        w[ 1 + k ] += ( unsigned long long )__popcll( m );
        w[ 2 + k ] += 1;
    }
}
#define ACN_TALLY( k, x ) phase_tally( k, x )
#define ACN_LAP( k ) phase_lap( k )
#define ACN_PHASE_INIT phase_init();
#define ACN_PHASE_FLUSH( counters, kernel ) phase_flush( counters, kernel );
#else
#define ACN_TALLY( k, x )
#define ACN_LAP( k )
#define ACN_PHASE_INIT
#define ACN_PHASE_FLUSH( counters, kernel )
#endif

/* the two read-only scene arrays, passed BY VALUE into the non-inlined machines (global address space, so the
 * scene struct is never forced into scratch) */
template< class NP > struct SceneRefT { NP nodes; const GNode ACN_CONST* gnodes; ElemP elems; uint32_t* flags; uint32_t n_elems; uint32_t lds_stack; };
template< class NP > __device__ __forceinline__ SceneRefT< NP > sref( const DevSceneT< NP >& sc ) { SceneRefT< NP > r; r.nodes = sc.nodes; r.gnodes = sc.gnodes; r.elems = sc.elems; r.flags = sc.flags; r.n_elems = sc.n_elems; r.lds_stack = sc.lds_stack; return r; }

#endif /* ACN_DEV_SCENE_H */
