/* k_lens_layers_merge.hip -- acn_lens_layers_merge* and acn_lens_layers_resolve_dev (include/actinon_hip.h states the class list, the
 * pair merge, the ranking, the rest and the coverage; tests/lens_layers_merge_model.py restates them in numpy and the two are
 * compared bit for bit).
 *
 *   k_lens_layers_merge    one position per lane.  The lane reads its index first; a skipped lane touches nothing.  It then reads the
 *                  part's five records (448 bytes), returns if its three statistics records are EMPTY, reads the accumulator's five
 *                  and only then stores: surface records as eight 16-byte pieces, statistics records as four, as k_surface and
 *                  k_stats_merge move theirs.  The class list is the four layer slots A0, A1, B0, B1 where they lie, each with a
 *                  `present` flag: an entry's place in the list is its slot number, a slot of the part that was merged into an earlier
 *                  entry leaves the list, and nothing is compacted.  Every choice among the slots is a chain of selects over
 *                  constant indices (layer_pick), so the slots stay in registers; the pair merge has two call sites, one for B0 and
 *                  one for B1.  No lane reads another lane's registers: a record depends on the six slots of its position alone.
 *   k_lens_layers_resolve  one position per lane, as k_stats_resolve: the three records folded into one, resolved by the same
 *                  function.
 * The statistics arithmetic is that of acn_stats_dev.h, which k_stats_merge runs too. */
#include <hip/hip_runtime.h>
#include "acn_launch.h"
#include "acn_stats_dev.h"
#include "acn_surfclass.h"

#define LAYER_PIECES ( ACN_SURF_STRIDE / 2 )
#define STATS_PIECES ( ACN_STATS_STRIDE / 2 )

/* a layer slot: its surface record as { dist, pos.x } { pos.y, pos.z } { nor.x, nor.y } { nor.z, e } { x, alb.x } { alb.y, alb.z }
 * { kind, h } { weight, coverage } and its statistics record */
struct Layer { double2 s[ LAYER_PIECES ]; StatsRec t; };

__device__ static inline Layer layer_load( const double2* __restrict__ surf, const double2* __restrict__ stats )
{
    Layer l;
    #pragma unroll
    for( int k = 0; k < LAYER_PIECES; k++ ) l.s[ k ] = surf[ k ];
    #pragma unroll
    for( int k = 0; k < STATS_PIECES; k++ ) l.t.q[ k ] = stats[ k ];
    return l;
}

__device__ static inline StatsRec stats_load( const double2* __restrict__ stats )
{
    StatsRec r;
    #pragma unroll
    for( int k = 0; k < STATS_PIECES; k++ ) r.q[ k ] = stats[ k ];
    return r;
}

__device__ static inline void stats_store( double2* stats, const StatsRec& r )
{
    #pragma unroll
    for( int k = 0; k < STATS_PIECES; k++ ) stats[ k ] = r.q[ k ];
}

__device__ static inline double2 pick2( bool c, double2 a, double2 b ) { return make_double2( c ? a.x : b.x, c ? a.y : b.y ); }

/* c ? a : b, piece by piece */
__device__ static inline StatsRec stats_pick( bool c, const StatsRec& a, const StatsRec& b )
{
    StatsRec r;
    #pragma unroll
    for( int k = 0; k < STATS_PIECES; k++ ) r.q[ k ] = pick2( c, a.q[ k ], b.q[ k ] );
    return r;
}

__device__ static inline Layer layer_pick( bool c, const Layer& a, const Layer& b )
{
    Layer r;
    #pragma unroll
    for( int k = 0; k < LAYER_PIECES; k++ ) r.s[ k ] = pick2( c, a.s[ k ], b.s[ k ] );
    r.t = stats_pick( c, a.t, b.t );
    return r;
}

__device__ static inline SurfKey layer_key( const Layer& l ) { return surf_key_of( l.s[ 0 ].x, l.s[ 3 ].y, l.s[ 4 ].x, l.s[ 6 ].y ); }

/* the absent layer of the split and its statistics record of eight zeros */
__device__ static inline Layer layer_absent()
{
    Layer l;
    const double2 zero = make_double2( 0.0, 0.0 );
    l.s[ 0 ] = make_double2( __builtin_inf(), 0.0 ); l.s[ 1 ] = zero; l.s[ 2 ] = zero; l.s[ 3 ] = make_double2( 0.0, -1.0 );
    l.s[ 4 ] = make_double2( -1.0, 0.0 ); l.s[ 5 ] = zero; l.s[ 6 ] = zero; l.s[ 7 ] = zero;
    l.t = stats_zero();
    return l;
}

/* PAIR MERGE of the header: b into the entry a, both PRESENT and of one key; hit: that key's.  [ 15 ] is a's and is set later */
__device__ static inline Layer layer_pair_merge( const Layer& a, const Layer& b, bool hit )
{
    Layer r;
    const double na = a.t.q[ 0 ].x, nb = b.t.q[ 0 ].x;
    const double f = nb / ( na + nb );
    const StatsRec t = stats_pair_merge( a.t, b.t );
    const double w = a.s[ 7 ].x + ( b.s[ 7 ].x - a.s[ 7 ].x ) * f;
    r.t = t;
    if( !hit )
    {
        r = layer_absent();
        r.t = t;
        r.s[ 6 ].y = a.s[ 6 ].y;
        r.s[ 7 ] = make_double2( w, a.s[ 7 ].y );
        return r;
    }
    const double gx = a.s[ 2 ].x + ( b.s[ 2 ].x - a.s[ 2 ].x ) * f;
    const double gy = a.s[ 2 ].y + ( b.s[ 2 ].y - a.s[ 2 ].y ) * f;
    const double gz = a.s[ 3 ].x + ( b.s[ 3 ].x - a.s[ 3 ].x ) * f;
    const double q = ( gx * gx + gy * gy ) + gz * gz;
    const double len = acn_sqrt( q );
    const bool has = q > 0;
    const uint32_t kinds = ( uint32_t )( int32_t )a.s[ 6 ].x | ( uint32_t )( int32_t )b.s[ 6 ].x;
    r.s[ 0 ] = make_double2( a.s[ 0 ].x + ( b.s[ 0 ].x - a.s[ 0 ].x ) * f, a.s[ 0 ].y + ( b.s[ 0 ].y - a.s[ 0 ].y ) * f );
    r.s[ 1 ] = make_double2( a.s[ 1 ].x + ( b.s[ 1 ].x - a.s[ 1 ].x ) * f, a.s[ 1 ].y + ( b.s[ 1 ].y - a.s[ 1 ].y ) * f );
    r.s[ 2 ] = make_double2( has ? gx / len : 0.0, has ? gy / len : 0.0 );
    r.s[ 3 ] = make_double2( has ? gz / len : 0.0, a.s[ 3 ].y );
    r.s[ 4 ] = make_double2( a.s[ 4 ].x, a.s[ 4 ].y + ( b.s[ 4 ].y - a.s[ 4 ].y ) * f );
    r.s[ 5 ] = make_double2( a.s[ 5 ].x + ( b.s[ 5 ].x - a.s[ 5 ].x ) * f, a.s[ 5 ].y + ( b.s[ 5 ].y - a.s[ 5 ].y ) * f );
    r.s[ 6 ] = make_double2( ( double )kinds, a.s[ 6 ].y );
    r.s[ 7 ] = make_double2( w, a.s[ 7 ].y );
    return r;
}

/* plane l of the surface records at surf + l * surf_plane, of the statistics records at stats + l * stats_plane (in double2) */
__global__ __launch_bounds__( 256 )
void k_lens_layers_merge( double2* acc_surf, double2* acc_stats, size_t n_acc, const double2* __restrict__ part_surf,
                          const double2* __restrict__ part_stats, size_t n_part, const long long* __restrict__ index )
{
    const size_t j = ( size_t )blockIdx.x * blockDim.x + threadIdx.x;
    if( j >= n_part ) return;
    long long i = ( long long )j;
    if( index )
    {
        i = index[ j ];
        if( i < 0 ) return;
    }
    if( ( size_t )i >= n_acc ) return;
    const size_t bs = n_part * LAYER_PIECES, bt = n_part * STATS_PIECES, as = n_acc * LAYER_PIECES, at = n_acc * STATS_PIECES;
    const double2* ps = part_surf + j * LAYER_PIECES;
    const double2* pt = part_stats + j * STATS_PIECES;
    Layer S2 = layer_load( ps, pt ), S3 = layer_load( ps + bs, pt + bt );
    const StatsRec Br = stats_load( pt + 2 * bt );
    bool p2 = !stats_empty( S2.t.q[ 0 ].x ), p3 = !stats_empty( S3.t.q[ 0 ].x );
    if( !p2 && !p3 && stats_empty( Br.q[ 0 ].x ) ) return;
    double2* qs = acc_surf + ( size_t )i * LAYER_PIECES;
    double2* qt = acc_stats + ( size_t )i * STATS_PIECES;
    Layer S0 = layer_load( qs, qt ), S1 = layer_load( qs + as, qt + at );
    const StatsRec Ar = stats_load( qt + 2 * at );
    const bool p0 = !stats_empty( S0.t.q[ 0 ].x ), p1 = !stats_empty( S1.t.q[ 0 ].x );
    const SurfKey k0 = layer_key( S0 ), k1 = layer_key( S1 ), k2 = layer_key( S2 ), k3 = layer_key( S3 );

    /* the class list: B0, then B1, into the first entry of its key */
    if( p2 )
    {
        const int t = ( p0 && surf_key_eq( k2, k0 ) ) ? 0 : ( p1 && surf_key_eq( k2, k1 ) ) ? 1 : -1;
        if( t >= 0 )
        {
            const Layer m = layer_pair_merge( layer_pick( t == 0, S0, S1 ), S2, ( k2.hh & 1u ) != 0 );
            S0 = layer_pick( t == 0, m, S0 );
            S1 = layer_pick( t == 1, m, S1 );
            p2 = false;
        }
    }
    if( p3 )
    {
        const int t = ( p0 && surf_key_eq( k3, k0 ) ) ? 0 : ( p1 && surf_key_eq( k3, k1 ) ) ? 1 : ( p2 && surf_key_eq( k3, k2 ) ) ? 2 : -1;
        if( t >= 0 )
        {
            const Layer m = layer_pair_merge( layer_pick( t == 0, S0, layer_pick( t == 1, S1, S2 ) ), S3, ( k3.hh & 1u ) != 0 );
            S0 = layer_pick( t == 0, m, S0 );
            S1 = layer_pick( t == 1, m, S1 );
            S2 = layer_pick( t == 2, m, S2 );
            p3 = false;
        }
    }

    /* the ranking: by n, descending; only a strictly larger n takes over from an earlier entry (a PRESENT n is >= 1) */
    const double n0 = S0.t.q[ 0 ].x, n1 = S1.t.q[ 0 ].x, n2 = S2.t.q[ 0 ].x, n3 = S3.t.q[ 0 ].x;
    int first = -1, second = -1, third = -1, fourth = -1;
    double best = 0.0;
    if( p0 ) { first = 0; best = n0; }
    if( p1 && n1 > best ) { first = 1; best = n1; }
    if( p2 && n2 > best ) { first = 2; best = n2; }
    if( p3 && n3 > best ) { first = 3; best = n3; }
    best = 0.0;
    if( p0 && first != 0 ) { second = 0; best = n0; }
    if( p1 && first != 1 && n1 > best ) { second = 1; best = n1; }
    if( p2 && first != 2 && n2 > best ) { second = 2; best = n2; }
    if( p3 && first != 3 && n3 > best ) { second = 3; best = n3; }
    best = 0.0;
    if( p0 && first != 0 && second != 0 ) { third = 0; best = n0; }
    if( p1 && first != 1 && second != 1 && n1 > best ) { third = 1; best = n1; }
    if( p2 && first != 2 && second != 2 && n2 > best ) { third = 2; best = n2; }
    if( p3 && first != 3 && second != 3 && n3 > best ) { third = 3; best = n3; }
    if( p0 && first != 0 && second != 0 && third != 0 ) fourth = 0;
    if( p1 && first != 1 && second != 1 && third != 1 ) fourth = 1;
    if( p2 && first != 2 && second != 2 && third != 2 ) fourth = 2;
    if( p3 && first != 3 && second != 3 && third != 3 ) fourth = 3;

    /* the rest: Ar, Br, the third and the fourth entry's statistics, folded in that order */
    StatsRec rest = stats_fold( Ar, Br );
    if( third >= 0 ) rest = stats_fold( rest, stats_pick( third == 0, S0.t, stats_pick( third == 1, S1.t, stats_pick( third == 2, S2.t, S3.t ) ) ) );
    if( fourth >= 0 ) rest = stats_fold( rest, stats_pick( fourth == 0, S0.t, stats_pick( fourth == 1, S1.t, stats_pick( fourth == 2, S2.t, S3.t ) ) ) );
    const bool rest_empty = stats_empty( rest.q[ 0 ].x );
    rest = stats_pick( rest_empty, stats_zero(), rest );

    /* the layers and their coverage */
    const Layer none = layer_absent();
    Layer L0 = layer_pick( first == 0, S0, layer_pick( first == 1, S1, layer_pick( first == 2, S2, layer_pick( first == 3, S3, none ) ) ) );
    Layer L1 = layer_pick( second == 0, S0, layer_pick( second == 1, S1, layer_pick( second == 2, S2, layer_pick( second == 3, S3, none ) ) ) );
    const double m0 = first >= 0 ? L0.t.q[ 0 ].x : 0.0, m1 = second >= 0 ? L1.t.q[ 0 ].x : 0.0, mr = rest_empty ? 0.0 : rest.q[ 0 ].x;
    const double Kp = ( m0 + m1 ) + mr;
    if( first >= 0 ) L0.s[ 7 ].y = m0 / Kp;
    if( second >= 0 ) L1.s[ 7 ].y = m1 / Kp;

    #pragma unroll
    for( int k = 0; k < LAYER_PIECES; k++ ) { qs[ k ] = L0.s[ k ]; qs[ as + k ] = L1.s[ k ]; }
    stats_store( qt, L0.t );
    stats_store( qt + at, L1.t );
    stats_store( qt + 2 * at, rest );
}

/* stats: plane l at stats + l * n * 4 pieces.  pooled = fold( fold( s0, s1 ), sr ), eight zeros when that is EMPTY */
__global__ __launch_bounds__( 256 )
void k_lens_layers_resolve( const double2* __restrict__ stats, size_t n, double bg_x, double bg_y, double bg_z, double gamma, int linear,
                            double* __restrict__ out_rgb, double* __restrict__ out_noise, double2* __restrict__ out_pooled )
{
    const size_t i = ( size_t )blockIdx.x * blockDim.x + threadIdx.x;
    if( i >= n ) return;
    const size_t plane = n * STATS_PIECES;
    const double2* p = stats + i * STATS_PIECES;
    const StatsRec s0 = stats_load( p ), s1 = stats_load( p + plane ), sr = stats_load( p + 2 * plane );
    StatsRec pooled = stats_fold( stats_fold( s0, s1 ), sr );
    pooled = stats_pick( stats_empty( pooled.q[ 0 ].x ), stats_zero(), pooled );
    stats_resolve_write( pooled, i, bg_x, bg_y, bg_z, gamma, linear, out_rgb, out_noise );
    if( out_pooled ) stats_store( out_pooled + i * STATS_PIECES, pooled );
}

void acn_launch_lens_layers_merge( double* acc_surface, double* acc_stats, size_t n_acc, const double* part_surface, const double* part_stats,
                                   size_t n_part, const int64_t* index, hipStream_t stream )
{
    hipLaunchKernelGGL( k_lens_layers_merge, dim3( ( unsigned )( ( n_part + 255 ) / 256 ) ), dim3( 256 ), 0, stream,
                        ( double2* )acc_surface, ( double2* )acc_stats, n_acc, ( const double2* )part_surface, ( const double2* )part_stats, n_part,
                        ( const long long* )index );
}

void acn_launch_lens_layers_resolve( const double* stats, size_t n, const double* background, double gamma, int linear, double* out_rgb,
                                     double* out_noise, double* out_pooled, hipStream_t stream )
{
    hipLaunchKernelGGL( k_lens_layers_resolve, dim3( ( unsigned )( ( n + 255 ) / 256 ) ), dim3( 256 ), 0, stream,
                        ( const double2* )stats, n, background[ 0 ], background[ 1 ], background[ 2 ], gamma, linear, out_rgb, out_noise,
                        ( double2* )out_pooled );
}
