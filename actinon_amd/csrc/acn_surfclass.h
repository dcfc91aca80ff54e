/* acn_surfclass.h -- the steps that the kernels which reduce the K surface records of a position share (k_lens_surface.hip,
 * k_lens_layers.hip; include/actinon_hip.h states the class and the record under acn_surface_reduce*): the class ( hit, e, x, h )
 * of a record as they compare it, the tile of a workgroup in LDS and its staging, the search for the dominant class, and double f
 * of the aggregate record.  Each kernel keeps its own LDS arrays and its own passes; every function here is inlined.
 *
 * The tile: a workgroup of 256 lanes takes SURF_TILE_POS consecutive positions, 16 lanes each, and holds SURF_TILE_K samples of
 * each at a time.  A row of a position is SURF_TILE_K + 1 records, so the rows of the two positions that share a group of 32 lanes
 * of an 8-byte read lie 128 bytes apart modulo the 256 bytes of the banks: no conflict. */
#ifndef ACN_SURFCLASS_H
#define ACN_SURFCLASS_H

#include <hip/hip_runtime.h>
#include <cstdint>
#include "acn_launch.h"

#define SURF_TILE_POS 16
#define SURF_TILE_K   16
#define SURF_ROW      ( ( SURF_TILE_K + 1 ) * ACN_SURF_STRIDE )   /* doubles of a position's row of records in LDS */
#define SURF_RAD_ROW  ( SURF_TILE_K * 3 )                         /* ... and of its row of radiances */
#define SURF_CLASSES  8
#define SURF_NO_K     0xFFFFFFFFu

/* positions of one launch: a multiple of the tile, far below the grid limit of 2^31 - 1 workgroups */
#define SURF_LAUNCH_POS ( ( size_t )1 << 30 )

/* the class of a sample as two words: ( e, x ) and ( h, hit ) */
struct SurfKey { uint64_t ex, hh; };

/* from doubles [ 0 ], [ 7 ], [ 8 ], [ 13 ] of a record (k_lens_layers_merge.hip holds its records in registers) */
__device__ static inline SurfKey surf_key_of( double dist, double de, double dx, double dh )
{
    SurfKey key;
    const uint32_t e = ( uint32_t )( int32_t )de, x = ( uint32_t )( int32_t )dx, h = ( uint32_t )( int32_t )dh;
    key.ex = ( ( uint64_t )e << 32 ) | x;
    key.hh = ( ( uint64_t )h << 1 ) | ( dist < __builtin_inf() ? 1u : 0u );
    return key;
}

__device__ static inline SurfKey surf_key( const double* r ) { return surf_key_of( r[ 0 ], r[ 7 ], r[ 8 ], r[ 13 ] ); }

__device__ static inline bool surf_key_eq( const SurfKey& a, const SurfKey& b ) { return a.ex == b.ex && a.hh == b.hh; }

/* the samples of a workgroup: where they come from, where they go in LDS and which of them are there */
struct SurfTile
{
    const double2* records; const double* rad;   /* [ position ][ k ][ 16 ] as 16-byte pieces; [ position ][ k ][ 3 ] or null */
    size_t p0; uint32_t np, K;                   /* the workgroup's positions [ p0, p0 + np ) of K samples each */
    double2* tile2; double* rtile;               /* rows of SURF_ROW / 2 pieces; rows of SURF_RAD_ROW doubles */
    uint32_t staged;                             /* the k0 of the tile in LDS, the same in every lane; SURF_NO_K: none */
};

/* samples [ k0, k0 + kc ) of the workgroup's positions -> LDS, unless they are there: the records, with RAD the radiances too,
 * consecutive lanes on consecutive pieces.  Every lane of the workgroup calls it */
template< bool RAD >
__device__ static inline void surf_stage( SurfTile& t, uint32_t k0, uint32_t kc )
{
    if( t.staged == k0 ) return;
    if( t.staged != SURF_NO_K ) __syncthreads();   /* (the reads of the tile before) */
    const uint32_t pieces = kc * ( ACN_SURF_STRIDE / 2 );
    for( uint32_t idx = threadIdx.x; idx < t.np * pieces; idx += 256 )
    {
        const uint32_t p = idx / pieces, r = idx - p * pieces;
        t.tile2[ p * ( SURF_ROW / 2 ) + r ] = t.records[ ( ( t.p0 + p ) * t.K + k0 ) * ( ACN_SURF_STRIDE / 2 ) + r ];
    }
    if constexpr( RAD )
    {
        const uint32_t words = kc * 3;
        for( uint32_t idx = threadIdx.x; idx < t.np * words; idx += 256 )
        {
            const uint32_t p = idx / words, r = idx - p * words;
            t.rtile[ p * SURF_RAD_ROW + r ] = t.rad[ ( ( t.p0 + p ) * t.K + k0 ) * 3 + r ];
        }
    }
    __syncthreads();
    t.staged = k0;
}

/* The dominant class of the samples of the lane's position (row: its row of the tile; mine: the position exists) from sample
 * `start` on (SURF_NO_K: nothing to search), with EXCLUDE of those outside the class `excluded`, whose members are counted nowhere
 * and take no place in the table: the class of most members, among equals the one that appears first; *cnt = 0: there is none.
 * Every lane walks the keys of its position's samples from LDS in the order of k -- the 16 lanes read the same addresses, which
 * the LDS broadcasts -- into a table of SURF_CLASSES classes (key, members, first k) in registers.  A sample that finds the table
 * full and its class not in it is where the next round starts: the rounds go on until no sample is left over, at most
 * K / SURF_CLASSES of them, and only the workgroups that hold such a position run them.  A class is counted whole in the round in
 * which it first appears (every round starts at or before that sample); a later round may count a part of it again, which has
 * fewer members and never wins.  So the class is exact for any K and any number of classes. */
template< bool RAD, bool EXCLUDE >
__device__ static inline void surf_dominant( SurfTile& t, const double* row, bool mine, uint32_t start, SurfKey excluded,
                                             SurfKey* best, uint32_t* cnt )
{
    SurfKey best_key; best_key.ex = 0; best_key.hh = 0;
    uint32_t best_cnt = 0, best_first = SURF_NO_K;
    bool more;
    do
    {
        SurfKey ckey[ SURF_CLASSES ];
        uint32_t ccnt[ SURF_CLASSES ], cfirst[ SURF_CLASSES ];
        #pragma unroll
        for( int j = 0; j < SURF_CLASSES; j++ ) { ckey[ j ].ex = 0; ckey[ j ].hh = 0; ccnt[ j ] = 0; cfirst[ j ] = SURF_NO_K; }
        uint32_t ncls = 0, next = SURF_NO_K;
        for( uint32_t k0 = 0; k0 < t.K; k0 += SURF_TILE_K )
        {
            const uint32_t kc = t.K - k0 < SURF_TILE_K ? t.K - k0 : SURF_TILE_K;
            surf_stage< RAD >( t, k0, kc );
            if( !mine || start == SURF_NO_K ) continue;
            for( uint32_t k = start > k0 ? start - k0 : 0; k < kc; k++ )
            {
                const SurfKey key = surf_key( row + k * ACN_SURF_STRIDE );
                if( EXCLUDE && surf_key_eq( key, excluded ) ) continue;
                bool found = false;
                #pragma unroll
                for( int j = 0; j < SURF_CLASSES; j++ )
                    if( ( uint32_t )j < ncls && surf_key_eq( ckey[ j ], key ) ) { ccnt[ j ]++; found = true; }
                if( found ) continue;
                if( ncls < SURF_CLASSES )
                {
                    #pragma unroll
                    for( int j = 0; j < SURF_CLASSES; j++ )
                        if( ( uint32_t )j == ncls ) { ckey[ j ] = key; ccnt[ j ] = 1; cfirst[ j ] = k0 + k; }
                    ncls++;
                }
                else if( next == SURF_NO_K ) next = k0 + k;
            }
        }
        #pragma unroll
        for( int j = 0; j < SURF_CLASSES; j++ )
            if( ( uint32_t )j < ncls && ( ccnt[ j ] > best_cnt || ( ccnt[ j ] == best_cnt && cfirst[ j ] < best_first ) ) )
            {
                best_key = ckey[ j ]; best_cnt = ccnt[ j ]; best_first = cfirst[ j ];
            }
        start = next;
        more = __syncthreads_or( mine && next != SURF_NO_K ) != 0;
    } while( more );
    *best = best_key; *cnt = best_cnt;
}

/* double f of the aggregate record over the m members of the class `key`: sum is the ordered sum of double f, kinds the OR of the
 * members' [ 12 ], gn the means of the normal's three components (read only where hit && m > 1), cover the [ 15 ] of the record */
__device__ static inline double surf_value( uint32_t f, const SurfKey& key, double sum, uint32_t m, uint32_t kinds, const double* gn, double cover )
{
    const bool hit = ( key.hh & 1u ) != 0;
    const double mean = sum / ( double )m;
    if( f == 15 ) return cover;
    if( f == 14 ) return mean;
    if( f == 13 ) return ( double )( int32_t )( uint32_t )( key.hh >> 1 );
    if( !hit ) return f == 0 ? __builtin_inf() : ( f == 7 || f == 8 ) ? -1.0 : 0.0;
    if( f == 7 ) return ( double )( int32_t )( uint32_t )( key.ex >> 32 );
    if( f == 8 ) return ( double )( int32_t )( uint32_t )key.ex;
    if( f == 12 ) return ( double )kinds;
    if( f >= 4 && f <= 6 && m > 1 )
    {
        const double gx = gn[ 0 ], gy = gn[ 1 ], gz = gn[ 2 ];
        const double q = ( gx * gx + gy * gy ) + gz * gz;
        return q > 0 ? mean / acn_sqrt( q ) : 0.0;
    }
    return mean;   /* (m == 1: sum / 1.0 is the sample's bits) */
}

#endif
