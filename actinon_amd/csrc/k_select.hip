/* k_select.hip -- the kernels of acn_select_above* and acn_key_histogram* (include/actinon_hip.h states the contract;
 * tests/select_model.py restates it in numpy and the two are compared bit for bit).
 *
 * A selection is three launches, and no workgroup of a launch reads a word another workgroup of that launch writes:
 *   k_select_count    one workgroup per tile of ACN_SELECT_TILE entries: how many of them are above the threshold
 *   k_select_scan     ONE workgroup turns the tile counts into their exclusive prefix sums, 1024 tiles per round with a carry, and
 *                     writes the total behind them
 *   k_select_scatter  one workgroup per tile again: it recomputes the predicate, ranks the lanes of a wave with __ballot / mbcnt,
 *                     the waves and rounds of the tile through LDS, adds the tile's prefix and writes the entries of rank < capacity
 * There is no single-pass look-back scan, no grid barrier and no loop that waits for another workgroup: a stalled wait is a hung
 * card, and all it would save is the second read of 8 bytes per entry.  The rank of an entry is the number of selected entries
 * before it, so a result depends on nothing but the keys: not on which entries share a wavefront, a workgroup or a tile, nor on the
 * order in which workgroups run.
 *
 * A tile is walked in rounds of 256 consecutive entries, lane t on entry t of the round, so loads are coalesced and the order of
 * the ranks is ( round, wave, lane ).
 *   k_key_hist        grid-stride loop on a bounded grid; counts per workgroup in LDS, then at most 257 64-bit integer atomics per
 *                     workgroup: exact, whatever the order */
#include <hip/hip_runtime.h>
#include "acn_launch.h"
#include "acn_select_host.h"

#define SEL_ROUNDS ( ACN_SELECT_TILE / 256u )
#define SEL_WAVES 4u
#define SEL_SCAN_PER_LANE 4u
#define HIST_MAX_GRID 512u

static_assert( ACN_SELECT_TILE >= 256u && ACN_SELECT_TILE <= 8192u && ( ACN_SELECT_TILE & ( ACN_SELECT_TILE - 1u ) ) == 0u, "tile size" );

/* (lanes_below: the mbcnt of acn_records.h) */

__global__ __launch_bounds__( 256 )
void k_select_count( const double* __restrict__ key, size_t n, double threshold, unsigned long long* __restrict__ tile_counts )
{
    __shared__ uint32_t wave_cnt[ SEL_WAVES ];
    const size_t t0 = ( size_t )blockIdx.x * ACN_SELECT_TILE;
    uint32_t c = 0;   /* of the wave: the same in all its lanes */
#pragma unroll
    for( uint32_t j = 0; j < SEL_ROUNDS; j++ )
    {
        const size_t i = t0 + j * 256u + threadIdx.x;
        const bool p = i < n && key[ i ] > threshold;
        c += ( uint32_t )__popcll( __ballot( p ) );
    }
    if( ( threadIdx.x & 63u ) == 0 ) wave_cnt[ threadIdx.x >> 6 ] = c;
    __syncthreads();
    if( threadIdx.x == 0 ) tile_counts[ blockIdx.x ] = ( unsigned long long )( ( wave_cnt[ 0 ] + wave_cnt[ 1 ] ) + ( wave_cnt[ 2 ] + wave_cnt[ 3 ] ) );
}

/* tiles[ i ] <- tiles[ 0 ] + ... + tiles[ i - 1 ], i < n_tiles; tiles[ n_tiles ] and *out_count (nullable) <- the total.  One workgroup */
__global__ __launch_bounds__( 256 )
void k_select_scan( unsigned long long* __restrict__ tiles, size_t n_tiles, unsigned long long* __restrict__ out_count )
{
    __shared__ unsigned long long part[ 256 ];
    const uint32_t tid = threadIdx.x;
    unsigned long long carry = 0;   /* the sum of the rounds before: the same in every lane */
    for( size_t base = 0; base < n_tiles; base += 256u * SEL_SCAN_PER_LANE )
    {
        const size_t i0 = base + ( size_t )tid * SEL_SCAN_PER_LANE;
        unsigned long long v[ SEL_SCAN_PER_LANE ], own = 0;
#pragma unroll
        for( uint32_t k = 0; k < SEL_SCAN_PER_LANE; k++ )
        {
            v[ k ] = i0 + k < n_tiles ? tiles[ i0 + k ] : 0ull;
            own += v[ k ];
        }
        part[ tid ] = own;
        __syncthreads();
        for( uint32_t off = 1; off < 256u; off <<= 1 )
        {
            const unsigned long long x = tid >= off ? part[ tid - off ] : 0ull;
            __syncthreads();
            part[ tid ] += x;
            __syncthreads();
        }
        unsigned long long run = carry + ( part[ tid ] - own );
        carry += part[ 255 ];
#pragma unroll
        for( uint32_t k = 0; k < SEL_SCAN_PER_LANE; k++ )
        {
            if( i0 + k < n_tiles ) tiles[ i0 + k ] = run;
            run += v[ k ];
        }
        __syncthreads();   /* part[ 255 ] is read before the next round writes it */
    }
    if( tid == 0 )
    {
        tiles[ n_tiles ] = carry;
        if( out_count ) *out_count = carry;
    }
}

__global__ __launch_bounds__( 256 )
void k_select_scatter( const double* __restrict__ key, size_t n, double threshold, const unsigned long long* __restrict__ tile_first,
                       unsigned long long capacity, const double* __restrict__ src_pos_xy, unsigned long long raster_width,
                       unsigned long long raster_first, long long* __restrict__ out_index, double* __restrict__ out_pos_xy )
{
    __shared__ uint32_t cnt[ SEL_ROUNDS * SEL_WAVES ];
    const unsigned long long first = tile_first[ blockIdx.x ];
    if( first >= capacity ) return;   /* (the whole workgroup: nothing of this tile is written) */
    const size_t t0 = ( size_t )blockIdx.x * ACN_SELECT_TILE;
    const uint32_t wave = threadIdx.x >> 6;
    uint32_t sel = 0, below[ SEL_ROUNDS ];
#pragma unroll
    for( uint32_t j = 0; j < SEL_ROUNDS; j++ )
    {
        const size_t i = t0 + j * 256u + threadIdx.x;
        const bool p = i < n && key[ i ] > threshold;
        const unsigned long long mask = __ballot( p );
        below[ j ] = lanes_below( mask );
        sel |= ( p ? 1u : 0u ) << j;
        if( ( threadIdx.x & 63u ) == 0 ) cnt[ j * SEL_WAVES + wave ] = ( uint32_t )__popcll( mask );
    }
    __syncthreads();
    uint32_t run = 0;   /* selected entries of the tile in the rounds before */
#pragma unroll
    for( uint32_t j = 0; j < SEL_ROUNDS; j++ )
    {
        uint32_t before = run;   /* ... and in the waves before of this round */
#pragma unroll
        for( uint32_t w = 0; w < SEL_WAVES; w++ )
        {
            const uint32_t c = cnt[ j * SEL_WAVES + w ];
            if( w < wave ) before += c;
            run += c;
        }
        const unsigned long long r = first + before + below[ j ];
        if( !( ( sel >> j ) & 1u ) || r >= capacity ) continue;
        const size_t i = t0 + j * 256u + threadIdx.x;
        if( out_index ) out_index[ r ] = ( long long )i;
        if( !out_pos_xy ) continue;
        double x, y;
        if( src_pos_xy ) { x = src_pos_xy[ 2 * i ]; y = src_pos_xy[ 2 * i + 1 ]; }
        else
        {
            const unsigned long long pix = raster_first + i;
            unsigned long long col, row;
            if( ( ( pix | raster_width ) >> 32 ) == 0 )   /* (the same quotient and remainder, without the 64-bit division) */
            {
                row = ( uint32_t )pix / ( uint32_t )raster_width;
                col = ( uint32_t )pix - ( uint32_t )row * ( uint32_t )raster_width;
            }
            else { row = pix / raster_width; col = pix - row * raster_width; }
            x = ( double )col + 0.5; y = ( double )row + 0.5;
        }
        out_pos_xy[ 2 * r ] = x; out_pos_xy[ 2 * r + 1 ] = y;
    }
}

__global__ __launch_bounds__( 256 )
void k_key_hist( const double* __restrict__ key, size_t n, unsigned long long* __restrict__ out_hist )
{
    __shared__ uint32_t bins[ ACN_KEY_HIST_WORDS ];   /* (a workgroup sees at most n <= 2^31 keys) */
    for( uint32_t b = threadIdx.x; b < ACN_KEY_HIST_WORDS; b += 256u ) bins[ b ] = 0u;
    __syncthreads();
    const size_t step = ( size_t )gridDim.x * 256u;
    for( size_t i = ( size_t )blockIdx.x * 256u + threadIdx.x; i < n; i += step )
        atomicAdd( &bins[ acn_select_key_bin( ( uint64_t )__double_as_longlong( key[ i ] ) ) ], 1u );
    __syncthreads();
    for( uint32_t b = threadIdx.x; b < ACN_KEY_HIST_WORDS; b += 256u )
        if( bins[ b ] ) atomicAdd( &out_hist[ b ], ( unsigned long long )bins[ b ] );
}

void acn_launch_select( const double* key, size_t n, double threshold, unsigned long long* tiles, unsigned long long capacity,
                        const double* src_pos_xy, unsigned long long raster_width, unsigned long long raster_first, int64_t* out_index,
                        double* out_pos_xy, unsigned long long* out_count, hipStream_t stream )
{
    const size_t n_tiles = ( size_t )acn_select_tiles( n );
    hipLaunchKernelGGL( k_select_count, dim3( ( unsigned )n_tiles ), dim3( 256 ), 0, stream, key, n, threshold, tiles );
    hipLaunchKernelGGL( k_select_scan, dim3( 1 ), dim3( 256 ), 0, stream, tiles, n_tiles, out_count );
    if( capacity && ( out_index || out_pos_xy ) )
        hipLaunchKernelGGL( k_select_scatter, dim3( ( unsigned )n_tiles ), dim3( 256 ), 0, stream, key, n, threshold,
                            ( const unsigned long long* )tiles, capacity, src_pos_xy, raster_width, raster_first, ( long long* )out_index, out_pos_xy );
}

void acn_launch_key_hist( const double* key, size_t n, unsigned long long* out_hist, hipStream_t stream )
{
    size_t grid = ( n + 2047 ) / 2048;   /* eight keys per lane before the grid is bounded */
    if( grid > HIST_MAX_GRID ) grid = HIST_MAX_GRID;
    hipLaunchKernelGGL( k_key_hist, dim3( ( unsigned )grid ), dim3( 256 ), 0, stream, key, n, out_hist );
}
