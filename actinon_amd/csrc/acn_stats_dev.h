/* acn_stats_dev.h -- the rules of the statistics record { n, mean.xyz, m2.xyz, 0 } that every kernel which reads one applies
 * (k_lens.hip, k_denoise.hip, k_denoise_layers.hip, k_lens_layers_merge.hip; include/actinon_hip.h states them under
 * ACN_STATS_STRIDE), and the merge of two records, which k_stats_merge and the layered merge and resolve share. */
#ifndef ACN_STATS_DEV_H
#define ACN_STATS_DEV_H

#include <hip/hip_runtime.h>
#include "acn_dev_image.h"   /* V3, cl_sat; acn_sqrt of acn_detmath.h */

/* a record whose [ 0 ] is not a finite number >= 1 is EMPTY (a NaN fails both comparisons) */
__device__ static inline bool stats_empty( double n ) { return !( n >= 1.0 && n < __builtin_inf() ); }

/* the variance of the mean of one channel: m2 its sum of squared deviations over the n > 1 samples of a record */
__device__ static inline double stats_var_of_mean( double m2, double n ) { return ( m2 / ( n - 1.0 ) ) / n; }

/* a record as the four 16-byte pieces it is moved in: { n, mean.x } { mean.y, mean.z } { m2.x, m2.y } { m2.z, 0 } */
struct StatsRec { double2 q[ 4 ]; };

__device__ static inline StatsRec stats_zero()
{
    StatsRec r;
    r.q[ 0 ] = r.q[ 1 ] = r.q[ 2 ] = r.q[ 3 ] = make_double2( 0.0, 0.0 );
    return r;
}

/* merge( a, b ) of acn_lens_stats_merge* where neither record is EMPTY */
__device__ static inline StatsRec stats_pair_merge( const StatsRec& a, const StatsRec& b )
{
    const double na = a.q[ 0 ].x, nb = b.q[ 0 ].x, nn = na + nb;
    const double fb = nb / nn, fab = ( na * nb ) / nn;
    const double dx = b.q[ 0 ].y - a.q[ 0 ].y, dy = b.q[ 1 ].x - a.q[ 1 ].x, dz = b.q[ 1 ].y - a.q[ 1 ].y;
    const double mx = a.q[ 0 ].y + dx * fb, my = a.q[ 1 ].x + dy * fb, mz = a.q[ 1 ].y + dz * fb;
    const double sx = ( a.q[ 2 ].x + b.q[ 2 ].x ) + ( dx * dx ) * fab;
    const double sy = ( a.q[ 2 ].y + b.q[ 2 ].y ) + ( dy * dy ) * fab;
    const double sz = ( a.q[ 3 ].x + b.q[ 3 ].x ) + ( dz * dz ) * fab;
    StatsRec r;
    r.q[ 0 ] = make_double2( nn, mx ); r.q[ 1 ] = make_double2( my, mz ); r.q[ 2 ] = make_double2( sx, sy ); r.q[ 3 ] = make_double2( sz, 0.0 );
    return r;
}

/* merge( a, b ) with the EMPTY rules: b EMPTY: a as it is; a EMPTY: b bit for bit */
__device__ static inline StatsRec stats_fold( const StatsRec& a, const StatsRec& b )
{
    if( stats_empty( b.q[ 0 ].x ) ) return a;
    if( stats_empty( a.q[ 0 ].x ) ) return b;
    return stats_pair_merge( a, b );
}

/* `noise` of a record: the standard error of the luminance relative to it; +inf for an EMPTY record and for n == 1 */
__device__ static inline double stats_noise( const StatsRec& r )
{
    const double cnt = r.q[ 0 ].x;
    if( stats_empty( cnt ) || !( cnt > 1.0 ) ) return __builtin_inf();
    const double vx = stats_var_of_mean( r.q[ 2 ].x, cnt ), vy = stats_var_of_mean( r.q[ 2 ].y, cnt ), vz = stats_var_of_mean( r.q[ 3 ].x, cnt );
    const double lum = ( 0.2126 * r.q[ 0 ].y + 0.7152 * r.q[ 1 ].x ) + 0.0722 * r.q[ 1 ].y;
    return acn_sqrt( ( ( 0.2126 * 0.2126 ) * vx + ( 0.7152 * 0.7152 ) * vy ) + ( 0.0722 * 0.0722 ) * vz ) / ( acn_fabs( lum ) + ACN_STATS_NOISE_FLOOR );
}

/* what a resolve writes for record i: out_rgb (nullable) the mean, or the background of an EMPTY record, through cl_s_sat unless
 * linear; out_noise (nullable) `noise` */
__device__ static inline void stats_resolve_write( const StatsRec& r, size_t i, double bg_x, double bg_y, double bg_z, double gamma, int linear,
                                                   double* __restrict__ out_rgb, double* __restrict__ out_noise )
{
    if( out_rgb )
    {
        V3 c = stats_empty( r.q[ 0 ].x ) ? mk( bg_x, bg_y, bg_z ) : mk( r.q[ 0 ].y, r.q[ 1 ].x, r.q[ 1 ].y );
        if( !linear ) c = cl_sat( c, gamma );
        out_rgb[ 3 * i ] = c.x; out_rgb[ 3 * i + 1 ] = c.y; out_rgb[ 3 * i + 2 ] = c.z;
    }
    if( out_noise ) out_noise[ i ] = stats_noise( r );
}

#endif
