/* k_lens_surface.hip -- the aggregate surface record of acn_surface_reduce* / acn_surface_lens* (include/actinon_hip.h states the
 * record; tests/lens_surface_model.py restates it in numpy and the two are compared bit for bit).
 *
 * records is [ position ][ k ][ 16 ]: the K records of a position are K * 128 contiguous bytes, so a lane that walked its position
 * alone would sit K * 128 bytes from its neighbour.  A workgroup therefore takes SURF_TILE_POS consecutive positions and copies
 * SURF_TILE_K records of each at a time into LDS as 16-byte pieces, consecutive lanes on consecutive pieces (with K <= SURF_TILE_K
 * the whole tile is one contiguous run, else runs of SURF_TILE_K * 128 bytes).  A position has 16 lanes, one per double of its
 * output record.  The steps are those of acn_surfclass.h, which k_lens_layers.hip runs too: surf_stage, surf_dominant, surf_value.
 *   pass 1  surf_dominant: the dominant class of the position's samples, exact for any K and any number of classes.
 *   pass 2  the tiles again (not when K <= SURF_TILE_K: the one tile is still in LDS); lane f adds double f of the members of the
 *           dominant class, alone and in the order of k, starting at the first member.  No lane reads another lane's registers and
 *           no sum is split: a record depends on its K input records alone.
 * The three lanes of the normal hand their means to each other through LDS; surf_value makes double f of the record; the records of
 * the workgroup are put together in LDS and leave as 16-byte pieces, consecutive lanes on consecutive pieces: 16 positions are one
 * run of 2 KiB.
 * LDS: 16 x 17 x 128 (rows padded, acn_surfclass.h) + 2 KiB + 384 = 37 KiB per workgroup, four workgroups per compute unit; the
 * kernel runs no CSG machine and takes no dynamic LDS. */
#include <hip/hip_runtime.h>
#include "acn_launch.h"
#include "acn_surfclass.h"

__global__ __launch_bounds__( 256 )
void k_surface_reduce( const double2* __restrict__ records, size_t n, uint32_t K, double2* __restrict__ out )
{
    __shared__ double2 tile2[ SURF_TILE_POS * SURF_ROW / 2 ];
    __shared__ double2 rec2[ SURF_TILE_POS * ACN_SURF_STRIDE / 2 ];
    __shared__ double gnor[ SURF_TILE_POS * 3 ];
    double* rec = ( double* )rec2;
    const size_t p0 = ( size_t )blockIdx.x * SURF_TILE_POS;
    const uint32_t np = n - p0 < SURF_TILE_POS ? ( uint32_t )( n - p0 ) : SURF_TILE_POS;
    const uint32_t tid = threadIdx.x;
    const uint32_t my_p = tid / ACN_SURF_STRIDE, my_f = tid % ACN_SURF_STRIDE;
    const bool mine = my_p < np;
    const double* row = ( const double* )tile2 + my_p * SURF_ROW;
    SurfTile t = { records, nullptr, p0, np, K, tile2, nullptr, SURF_NO_K };

    /* pass 1: the dominant class */
    SurfKey best_key;
    uint32_t best_cnt;
    surf_dominant< false, false >( t, row, mine, 0, SurfKey{ 0, 0 }, &best_key, &best_cnt );

    /* pass 2: the ordered sums over the members */
    double sum = 0.0;
    uint32_t kinds = 0, m = 0;
    for( uint32_t k0 = 0; k0 < K; k0 += SURF_TILE_K )
    {
        const uint32_t kc = K - k0 < SURF_TILE_K ? K - k0 : SURF_TILE_K;
        surf_stage< false >( t, k0, kc );
        if( !mine ) continue;
        for( uint32_t k = 0; k < kc; k++ )
        {
            const double* r = row + k * ACN_SURF_STRIDE;
            if( !surf_key_eq( surf_key( r ), best_key ) ) continue;
            const double v = r[ my_f ];
            sum = m ? sum + v : v;
            if( my_f == 12 ) kinds |= ( uint32_t )( int32_t )v;
            m++;
        }
    }

    /* the record.  The means of the normal's components go through LDS first */
    if( mine && ( best_key.hh & 1u ) && my_f >= 4 && my_f <= 6 && m > 1 ) gnor[ my_p * 3 + ( my_f - 4 ) ] = sum / ( double )m;
    __syncthreads();
    if( mine ) rec[ tid ] = surf_value( my_f, best_key, sum, m, kinds, gnor + my_p * 3, ( double )m / ( double )K );
    __syncthreads();
    if( tid < np * ( ACN_SURF_STRIDE / 2 ) ) out[ p0 * ( ACN_SURF_STRIDE / 2 ) + tid ] = rec2[ tid ];
}

void acn_launch_surface_reduce( const double* records, size_t n, uint32_t samples, double* out, hipStream_t stream )
{
    for( size_t first = 0; first < n; first += SURF_LAUNCH_POS )
    {
        const size_t cnt = n - first < SURF_LAUNCH_POS ? n - first : SURF_LAUNCH_POS;
        hipLaunchKernelGGL( k_surface_reduce, dim3( ( unsigned )( ( cnt + SURF_TILE_POS - 1 ) / SURF_TILE_POS ) ), dim3( 256 ), 0, stream,
                            ( const double2* )( records + first * samples * ( size_t )ACN_SURF_STRIDE ), cnt, samples,
                            ( double2* )( out + first * ( size_t )ACN_SURF_STRIDE ) );
    }
}
