/* k_lens_surface.hip -- the aggregate surface record of acn_surface_reduce* / acn_surface_lens* (include/actinon_hip.h states the
 * record; tests/lens_surface_model.py restates it in numpy and the two are compared bit for bit).
 *
 * records is [ position ][ k ][ 16 ]: the K records of a position are K * 128 contiguous bytes, so a lane that walked its position
 * alone would sit K * 128 bytes from its neighbour.  A workgroup therefore takes SURF_TILE_POS consecutive positions and copies
 * SURF_TILE_K records of each at a time into LDS as 16-byte pieces, consecutive lanes on consecutive pieces (with K <= SURF_TILE_K
 * the whole tile is one contiguous run, else runs of SURF_TILE_K * 128 bytes).  A position has 16 lanes, one per double of its
 * output record.
 *   pass 1  every lane of a position walks the keys ( hit, e, x, h ) of its samples from LDS in the order of k -- the 16 lanes read
 *           the same addresses, which the LDS broadcasts -- into a table of SURF_CLASSES classes (key, members, first k) in registers.
 *           A sample that finds the table full and its class not in it is where the next round starts: the rounds go on until no
 *           sample is left over, at most K / SURF_CLASSES of them, and only the workgroups that hold such a position run them.  A
 *           class is counted whole in the round in which it first appears (every round starts at or before that sample); a later
 *           round may count a part of it again, which has fewer members and never wins.  So the dominant class is exact for any K
 *           and any number of classes.
 *   pass 2  the tiles again (not when K <= SURF_TILE_K: the one tile is still in LDS); lane f adds double f of the members of the
 *           dominant class, alone and in the order of k, starting at the first member.  No lane reads another lane's registers and
 *           no sum is split: a record depends on its K input records alone.
 * The three lanes of the normal hand their means to each other through LDS; the records of the workgroup are put together in LDS
 * and leave as 16-byte pieces, consecutive lanes on consecutive pieces: 16 positions are one run of 2 KiB.
 * LDS: a row of a position is SURF_TILE_K + 1 records, so the rows of the two positions that share a group of 32 lanes of an
 * 8-byte read lie 128 bytes apart modulo the 256 bytes of the banks: no conflict.  16 x 17 x 128 + 2 KiB + 384 = 37 KiB per workgroup,
 * four workgroups per compute unit; the kernel runs no CSG machine and takes no dynamic LDS. */
#include <hip/hip_runtime.h>
#include "acn_launch.h"
#include "acn_surfclass.h"

#define SURF_TILE_POS 16
#define SURF_TILE_K   16
#define SURF_ROW      ( ( SURF_TILE_K + 1 ) * ACN_SURF_STRIDE )   /* doubles of a position's row in LDS */
#define SURF_CLASSES  8
#define SURF_NO_K     0xFFFFFFFFu

/* positions of one launch: a multiple of the tile, far below the grid limit of 2^31 - 1 workgroups */
#define SURF_REDUCE_LAUNCH_POS ( ( size_t )1 << 30 )

__global__ __launch_bounds__( 256 )
void k_surface_reduce( const double2* __restrict__ records, size_t n, uint32_t K, double2* __restrict__ out )
{
    __shared__ double2 tile2[ SURF_TILE_POS * SURF_ROW / 2 ];
    __shared__ double2 rec2[ SURF_TILE_POS * ACN_SURF_STRIDE / 2 ];
    __shared__ double gnor[ SURF_TILE_POS * 3 ];
    const double* tile = ( const double* )tile2;
    double* rec = ( double* )rec2;
    const size_t p0 = ( size_t )blockIdx.x * SURF_TILE_POS;
    const uint32_t np = n - p0 < SURF_TILE_POS ? ( uint32_t )( n - p0 ) : SURF_TILE_POS;
    const uint32_t tid = threadIdx.x;
    const uint32_t my_p = tid / ACN_SURF_STRIDE, my_f = tid % ACN_SURF_STRIDE;
    const bool mine = my_p < np;
    const double* row = tile + my_p * SURF_ROW;

    uint32_t staged = SURF_NO_K;   /* the k0 of the tile in LDS: the same in every lane */
    /* samples [ k0, k0 + kc ) of the workgroup's positions -> LDS, unless they are there */
    #define SURF_STAGE( k0, kc ) \
        if( staged != ( k0 ) ) \
        { \
            if( staged != SURF_NO_K ) __syncthreads();   /* (the reads of the tile before) */ \
            const uint32_t pieces = ( kc ) * ( ACN_SURF_STRIDE / 2 ); \
            for( uint32_t idx = tid; idx < np * pieces; idx += 256 ) \
            { \
                const uint32_t p = idx / pieces, r = idx - p * pieces; \
                tile2[ p * ( SURF_ROW / 2 ) + r ] = records[ ( ( p0 + p ) * K + ( k0 ) ) * ( ACN_SURF_STRIDE / 2 ) + r ]; \
            } \
            __syncthreads(); \
            staged = ( k0 ); \
        }

    /* pass 1: the dominant class */
    SurfKey best_key; best_key.ex = 0; best_key.hh = 0;
    uint32_t best_cnt = 0, best_first = SURF_NO_K;
    uint32_t start = 0;
    bool more;
    do
    {
        SurfKey ckey[ SURF_CLASSES ];
        uint32_t ccnt[ SURF_CLASSES ], cfirst[ SURF_CLASSES ];
        #pragma unroll
        for( int j = 0; j < SURF_CLASSES; j++ ) { ckey[ j ].ex = 0; ckey[ j ].hh = 0; ccnt[ j ] = 0; cfirst[ j ] = SURF_NO_K; }
        uint32_t ncls = 0, next = SURF_NO_K;
        for( uint32_t k0 = 0; k0 < K; k0 += SURF_TILE_K )
        {
            const uint32_t kc = K - k0 < SURF_TILE_K ? K - k0 : SURF_TILE_K;
            SURF_STAGE( k0, kc )
            if( !mine || start == SURF_NO_K ) continue;
            for( uint32_t k = start > k0 ? start - k0 : 0; k < kc; k++ )
            {
                const SurfKey key = surf_key( row + k * ACN_SURF_STRIDE );
                bool found = false;
                #pragma unroll
                for( int j = 0; j < SURF_CLASSES; j++ )
                    if( ( uint32_t )j < ncls && ckey[ j ].ex == key.ex && ckey[ j ].hh == key.hh ) { ccnt[ j ]++; found = true; }
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

    /* pass 2: the ordered sums over the members */
    double sum = 0.0;
    uint32_t kinds = 0, m = 0;
    for( uint32_t k0 = 0; k0 < K; k0 += SURF_TILE_K )
    {
        const uint32_t kc = K - k0 < SURF_TILE_K ? K - k0 : SURF_TILE_K;
        SURF_STAGE( k0, kc )
        if( !mine ) continue;
        for( uint32_t k = 0; k < kc; k++ )
        {
            const double* r = row + k * ACN_SURF_STRIDE;
            const SurfKey key = surf_key( r );
            if( key.ex != best_key.ex || key.hh != best_key.hh ) continue;
            const double v = r[ my_f ];
            sum = m ? sum + v : v;
            if( my_f == 12 ) kinds |= ( uint32_t )( int32_t )v;
            m++;
        }
    }
    #undef SURF_STAGE

    const bool hit = ( best_key.hh & 1u ) != 0;
    const bool is_nor = my_f >= 4 && my_f <= 6;
    const double mean = mine ? sum / ( double )m : 0.0;
    if( mine && hit && is_nor && m > 1 ) gnor[ my_p * 3 + ( my_f - 4 ) ] = mean;
    __syncthreads();
    if( mine )
    {
        double v;
        if( my_f == 15 ) v = ( double )m / ( double )K;
        else if( my_f == 14 ) v = mean;
        else if( my_f == 13 ) v = ( double )( int32_t )( uint32_t )( best_key.hh >> 1 );
        else if( !hit ) v = my_f == 0 ? __builtin_inf() : ( my_f == 7 || my_f == 8 ) ? -1.0 : 0.0;
        else if( my_f == 7 ) v = ( double )( int32_t )( uint32_t )( best_key.ex >> 32 );
        else if( my_f == 8 ) v = ( double )( int32_t )( uint32_t )best_key.ex;
        else if( my_f == 12 ) v = ( double )kinds;
        else if( is_nor && m > 1 )
        {
            const double gx = gnor[ my_p * 3 ], gy = gnor[ my_p * 3 + 1 ], gz = gnor[ my_p * 3 + 2 ];
            const double q = ( gx * gx + gy * gy ) + gz * gz;
            v = q > 0 ? mean / acn_sqrt( q ) : 0.0;
        }
        else v = mean;   /* (m == 1: sum / 1.0 is the sample's bits) */
        rec[ tid ] = v;
    }
    __syncthreads();
    if( tid < np * ( ACN_SURF_STRIDE / 2 ) ) out[ p0 * ( ACN_SURF_STRIDE / 2 ) + tid ] = rec2[ tid ];
}

void acn_launch_surface_reduce( const double* records, size_t n, uint32_t samples, double* out, hipStream_t stream )
{
    for( size_t first = 0; first < n; first += SURF_REDUCE_LAUNCH_POS )
    {
        const size_t cnt = n - first < SURF_REDUCE_LAUNCH_POS ? n - first : SURF_REDUCE_LAUNCH_POS;
        hipLaunchKernelGGL( k_surface_reduce, dim3( ( unsigned )( ( cnt + SURF_TILE_POS - 1 ) / SURF_TILE_POS ) ), dim3( 256 ), 0, stream,
                            ( const double2* )( records + first * samples * ( size_t )ACN_SURF_STRIDE ), cnt, samples,
                            ( double2* )( out + first * ( size_t )ACN_SURF_STRIDE ) );
    }
}
