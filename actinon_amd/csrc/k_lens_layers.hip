/* k_lens_layers.hip -- the layered records of acn_lens_layers_reduce* / acn_render_lens_layers* (include/actinon_hip.h states the
 * split and both records; tests/lens_layers_model.py restates them in numpy and the two are compared bit for bit).
 *
 * The arrangement and the steps are those of acn_surfclass.h, which k_surface_reduce (k_lens_surface.hip) runs too: a workgroup
 * takes SURF_TILE_POS consecutive positions and surf_stage copies SURF_TILE_K samples of each at a time into LDS -- the surface
 * records as 16-byte pieces, the radiances as doubles, consecutive lanes on consecutive pieces -- and a position has 16 lanes.
 *   pass 1  surf_dominant twice: the dominant class of all samples (layer 0), then, with its exclusion, the dominant class of the
 *           samples outside layer 0 (layer 1).  Either class is exact for any K and any number of classes.
 *   pass 2  lane f adds double f of the members of layer 0 and, apart, of layer 1, alone and in the order of k, each sum starting at
 *           its first member; lanes 0 .. 8 are also ( part, channel ) = ( f / 3, f % 3 ) of the statistics -- part 0, 1 the layers,
 *           2 the rest -- and add that channel of their part's radiances to +0.0 in the order of k.
 *   pass 3  lanes 0 .. 8 again over the samples: the squared deviations from the mean of pass 2, added to +0.0 in the order of k.
 * With K <= SURF_TILE_K the one tile stays in LDS for all passes.  No lane reads another lane's registers and no sum is split: a
 * record depends on the K records and K radiances of its position alone.  The three lanes of a normal hand their means to each other
 * through LDS; surf_value makes double f of either surface record -- plane 0 is the record of k_surface_reduce because it is made by
 * the same steps --; the records of the workgroup are put together in LDS and leave as 16-byte pieces, consecutive lanes on
 * consecutive pieces.
 * LDS: 16 x 17 x 128 (records, rows padded: acn_surfclass.h) + 16 x 16 x 24 (radiances) + 4 KiB + 3 KiB (the records that leave)
 * + 768 (normals) = 48 KiB per workgroup, three workgroups per compute unit; no CSG machine runs and no dynamic LDS is taken. */
#include <hip/hip_runtime.h>
#include "acn_launch.h"
#include "acn_surfclass.h"

/* out_surf: plane l at out_surf + l * surf_plane, out_stats: plane l at out_stats + l * stats_plane (both counted in double2) */
__global__ __launch_bounds__( 256 )
void k_lens_layers( const double2* __restrict__ records, const double* __restrict__ rad, size_t n, uint32_t K,
                    double2* __restrict__ out_surf, size_t surf_plane, double2* __restrict__ out_stats, size_t stats_plane )
{
    __shared__ double2 tile2[ SURF_TILE_POS * SURF_ROW / 2 ];
    __shared__ double rtile[ SURF_TILE_POS * SURF_RAD_ROW ];
    __shared__ double2 srec2[ 2 ][ SURF_TILE_POS * ACN_SURF_STRIDE / 2 ];
    __shared__ double2 trec2[ 3 ][ SURF_TILE_POS * ACN_STATS_STRIDE / 2 ];
    __shared__ double gnor[ 2 ][ SURF_TILE_POS * 3 ];
    const size_t p0 = ( size_t )blockIdx.x * SURF_TILE_POS;
    const uint32_t np = n - p0 < SURF_TILE_POS ? ( uint32_t )( n - p0 ) : SURF_TILE_POS;
    const uint32_t tid = threadIdx.x;
    const uint32_t my_p = tid / ACN_SURF_STRIDE, my_f = tid % ACN_SURF_STRIDE;
    const bool mine = my_p < np;
    const double* row = ( const double* )tile2 + my_p * SURF_ROW;
    const double* rrow = rtile + my_p * SURF_RAD_ROW;
    SurfTile t = { records, rad, p0, np, K, tile2, rtile, SURF_NO_K };

    /* pass 1: the dominant class of all samples, then of those outside it (nothing outside layer 0: nothing to search) */
    SurfKey lkey[ 2 ];
    uint32_t lcnt[ 2 ];
    surf_dominant< true, false >( t, row, mine, 0, SurfKey{ 0, 0 }, &lkey[ 0 ], &lcnt[ 0 ] );
    surf_dominant< true, true >( t, row, mine, lcnt[ 0 ] == K ? SURF_NO_K : 0, lkey[ 0 ], &lkey[ 1 ], &lcnt[ 1 ] );
    const bool have1 = lcnt[ 1 ] != 0;

    /* pass 2: the ordered sums over the members of either layer, and of the radiances of the lane's part */
    const bool stat_lane = my_f < 9;
    const uint32_t my_part = my_f / 3, my_c = my_f - my_part * 3;
    double sum[ 2 ] = { 0.0, 0.0 }, rsum = 0.0;
    uint32_t kinds[ 2 ] = { 0, 0 }, m[ 2 ] = { 0, 0 };
    for( uint32_t k0 = 0; k0 < K; k0 += SURF_TILE_K )
    {
        const uint32_t kc = K - k0 < SURF_TILE_K ? K - k0 : SURF_TILE_K;
        surf_stage< true >( t, k0, kc );
        if( !mine ) continue;
        for( uint32_t k = 0; k < kc; k++ )
        {
            const double* r = row + k * ACN_SURF_STRIDE;
            const SurfKey key = surf_key( r );
            const uint32_t part = surf_key_eq( key, lkey[ 0 ] ) ? 0u : ( have1 && surf_key_eq( key, lkey[ 1 ] ) ) ? 1u : 2u;
            const double v = r[ my_f ];
            #pragma unroll
            for( uint32_t l = 0; l < 2; l++ )
                if( part == l )
                {
                    sum[ l ] = m[ l ] ? sum[ l ] + v : v;
                    if( my_f == 12 ) kinds[ l ] |= ( uint32_t )( int32_t )v;
                    m[ l ]++;
                }
            if( stat_lane && part == my_part ) rsum = rsum + rrow[ k * 3 + my_c ];
        }
    }
    /* members of the lane's part of the statistics; the rest has what the layers leave */
    const uint32_t pm = my_part == 0 ? m[ 0 ] : my_part == 1 ? m[ 1 ] : K - m[ 0 ] - m[ 1 ];
    const double rmean = rsum / ( double )pm;

    /* pass 3: the squared deviations */
    double m2 = 0.0;
    for( uint32_t k0 = 0; k0 < K; k0 += SURF_TILE_K )
    {
        const uint32_t kc = K - k0 < SURF_TILE_K ? K - k0 : SURF_TILE_K;
        surf_stage< true >( t, k0, kc );
        if( !mine || !stat_lane ) continue;
        for( uint32_t k = 0; k < kc; k++ )
        {
            const SurfKey key = surf_key( row + k * ACN_SURF_STRIDE );
            const uint32_t part = surf_key_eq( key, lkey[ 0 ] ) ? 0u : ( have1 && surf_key_eq( key, lkey[ 1 ] ) ) ? 1u : 2u;
            if( part != my_part ) continue;
            const double d = rrow[ k * 3 + my_c ] - rmean;
            m2 = m2 + d * d;
        }
    }

    /* the records.  The means of the normals' components go through LDS first */
    const bool is_nor = my_f >= 4 && my_f <= 6;
    #pragma unroll
    for( uint32_t l = 0; l < 2; l++ )
        if( mine && is_nor && m[ l ] > 1 && ( lkey[ l ].hh & 1u ) ) gnor[ l ][ my_p * 3 + ( my_f - 4 ) ] = sum[ l ] / ( double )m[ l ];
    __syncthreads();
    if( mine )
    {
        double* s0 = ( double* )srec2[ 0 ];
        double* s1 = ( double* )srec2[ 1 ];
        s0[ tid ] = surf_value( my_f, lkey[ 0 ], sum[ 0 ], m[ 0 ], kinds[ 0 ], gnor[ 0 ] + my_p * 3, ( double )m[ 0 ] / ( double )K );
        if( have1 ) s1[ tid ] = surf_value( my_f, lkey[ 1 ], sum[ 1 ], m[ 1 ], kinds[ 1 ], gnor[ 1 ] + my_p * 3, ( double )m[ 1 ] / ( double )K );
        else s1[ tid ] = my_f == 0 ? __builtin_inf() : ( my_f == 7 || my_f == 8 ) ? -1.0 : 0.0;   /* absent: the miss record, [ 13 .. 15 ] zero */
        if( stat_lane )
        {
            double* t = ( double* )trec2[ my_part ] + my_p * ACN_STATS_STRIDE;
            t[ 1 + my_c ] = pm ? rmean : 0.0;
            t[ 4 + my_c ] = pm ? m2 : 0.0;
            if( my_c == 0 ) { t[ 0 ] = ( double )pm; t[ 7 ] = 0.0; }
        }
    }
    __syncthreads();
    if( tid < np * ( ACN_SURF_STRIDE / 2 ) )
    {
        out_surf[ p0 * ( ACN_SURF_STRIDE / 2 ) + tid ] = srec2[ 0 ][ tid ];
        out_surf[ surf_plane + p0 * ( ACN_SURF_STRIDE / 2 ) + tid ] = srec2[ 1 ][ tid ];
    }
    if( tid < np * ( ACN_STATS_STRIDE / 2 ) )
    {
        #pragma unroll
        for( uint32_t l = 0; l < 3; l++ ) out_stats[ l * stats_plane + p0 * ( ACN_STATS_STRIDE / 2 ) + tid ] = trec2[ l ][ tid ];
    }
}

void acn_launch_lens_layers( const double* records, const double* rad, size_t n, uint32_t samples, double* out_surface, size_t surface_plane,
                             double* out_stats, size_t stats_plane, hipStream_t stream )
{
    for( size_t first = 0; first < n; first += SURF_LAUNCH_POS )
    {
        const size_t cnt = n - first < SURF_LAUNCH_POS ? n - first : SURF_LAUNCH_POS;
        hipLaunchKernelGGL( k_lens_layers, dim3( ( unsigned )( ( cnt + SURF_TILE_POS - 1 ) / SURF_TILE_POS ) ), dim3( 256 ), 0, stream,
                            ( const double2* )( records + first * samples * ( size_t )ACN_SURF_STRIDE ), rad + first * samples * ( size_t )3, cnt, samples,
                            ( double2* )( out_surface + first * ( size_t )ACN_SURF_STRIDE ), surface_plane * ( ACN_SURF_STRIDE / 2 ),
                            ( double2* )( out_stats + first * ( size_t )ACN_STATS_STRIDE ), stats_plane * ( ACN_STATS_STRIDE / 2 ) );
    }
}
