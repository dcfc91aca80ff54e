/* k_frame.hip -- the kernels of the device-resident frame (include/actinon_hip.h states the contract, acn_frame_host.h holds every
 * expression once for host and device, tests/frame_model.py restates them in numpy and the three are compared bit for bit).
 *
 *   k_frame_key            the gradient key of every pixel.  One workgroup per tile of 32 x 8 pixels: it reads the records of the tile
 *                          and of a halo one pixel wide once (the 32 bytes of a record the key needs, as two 16-byte loads), keeps
 *                          their averages in LDS as three planes of doubles (a wave's row of a plane is 64 consecutive dwords: no
 *                          bank is asked twice) and every lane folds its eight neighbours in the driver's order.  A neighbour
 *                          outside the raster is decided from its coordinates, not from LDS
 *   k_frame_jitter         the positions of a slice of a plan: each lane jumps to its entry's place in the lcg00 stream
 *   k_frame_foreign_scan   the entries of a plan whose target is another pixel than their own: counted, and listed while slots last.
 *                          The one atomic of this unit; the order of the list means nothing
 *   k_frame_foreign_apply  ONE lane adds them in ascending entry number: from the list (the next larger entry each time), or, when
 *                          there were more than slots, by walking the whole plan.  No foreign entry: it returns at once
 *   k_frame_push           one lane per flagged pixel of a slice: the record in registers, its own entries in order k, three 16-byte
 *                          stores
 *   k_frame_image          averages and their 8-bit values
 * All of it is bound by memory; nothing here waits for another workgroup. */
#include <hip/hip_runtime.h>
#include "acn_launch.h"
#include "acn_frame_host.h"

#define KEY_TW 32
#define KEY_TH 8
#define KEY_HW ( KEY_TW + 2 )
#define KEY_HH ( KEY_TH + 2 )
#define KEY_CELLS ( KEY_HW * KEY_HH )

__global__ __launch_bounds__( 256 )
void k_frame_key( const double* __restrict__ acc, uint32_t width, uint32_t height, uint32_t tiles_x, double* __restrict__ key )
{
    __shared__ double avg[ 3 ][ KEY_CELLS ];
    const uint32_t tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
    const int64_t x0 = ( int64_t )tile_x * KEY_TW - 1, y0 = ( int64_t )tile_y * KEY_TH - 1;   /* the halo's corner */
    for( uint32_t c = threadIdx.x; c < KEY_CELLS; c += 256u )
    {
        const uint32_t cy = c / KEY_HW, cx = c - cy * KEY_HW;
        const int64_t x = x0 + cx, y = y0 + cy;
        double a[ 3 ] = { 0.0, 0.0, 0.0 };
        if( x >= 0 && x < ( int64_t )width && y >= 0 && y < ( int64_t )height )
        {
            const double2* r = ( const double2* )( acc + 6 * ( ( size_t )y * width + ( size_t )x ) );
            const double2 lo = r[ 1 ], hi = r[ 2 ];
            const double rec[ 6 ] = { 0.0, 0.0, lo.x, lo.y, hi.x, hi.y };
            acn_frame_avg( rec, a );
        }
        avg[ 0 ][ c ] = a[ 0 ]; avg[ 1 ][ c ] = a[ 1 ]; avg[ 2 ][ c ] = a[ 2 ];
    }
    __syncthreads();
    const uint32_t lx = threadIdx.x & ( KEY_TW - 1 ), ly = threadIdx.x / KEY_TW;
    const int64_t x = x0 + 1 + lx, y = y0 + 1 + ly;
    if( x >= ( int64_t )width || y >= ( int64_t )height ) return;
    const uint32_t c0 = ( ly + 1 ) * KEY_HW + ( lx + 1 );
    const double v[ 3 ] = { avg[ 0 ][ c0 ], avg[ 1 ][ c0 ], avg[ 2 ][ c0 ] };
    double g0 = 0;
#pragma unroll
    for( int k = 0; k < ACN_FRAME_NEIGHBOURS; k++ )
    {
        const int dx = ACN_FRAME_NB_DX( k ), dy = ACN_FRAME_NB_DY( k );
        const int64_t nx = x + dx, ny = y + dy;
        double g1 = 0;
        if( nx >= 0 && nx < ( int64_t )width && ny >= 0 && ny < ( int64_t )height )
        {
            const uint32_t c = ( uint32_t )( ( int )c0 + dy * KEY_HW + dx );
            const double n[ 3 ] = { avg[ 0 ][ c ], avg[ 1 ][ c ], avg[ 2 ][ c ] };
            g1 = acn_frame_clr_dev( v, n );
        }
        g0 = acn_frame_grad_max( g0, g1 );
    }
    key[ ( size_t )y * width + ( size_t )x ] = g0;
}

/* entries [ e0, e0 + cnt ) of a plan; index == nullptr: the main pass, entry e is the centre of pixel e */
__global__ __launch_bounds__( 256 )
void k_frame_jitter( const long long* __restrict__ index, uint64_t e0, uint64_t cnt, uint64_t samples, uint64_t rval, uint64_t width,
                     double* __restrict__ pos_xy )
{
    const uint64_t t = ( uint64_t )blockIdx.x * 256u + threadIdx.x;
    if( t >= cnt ) return;
    const uint64_t e = e0 + t;
    double p[ 2 ];
    if( !index )
    {
        const uint64_t j = e / width, i = e - j * width;
        p[ 0 ] = ( double )( int64_t )i + 0.5; p[ 1 ] = ( double )( int64_t )j + 0.5;
    }
    else
    {
        const uint64_t pix = ( uint64_t )index[ e / samples ];
        const uint64_t j = pix / width, i = pix - j * width;
        acn_frame_position( rval, e, i, j, p );
    }
    *( double2* )( pos_xy + 2 * e ) = make_double2( p[ 0 ], p[ 1 ] );
}

/* foreign[ 0 ]: the number of foreign entries (zeroed by the launch wrapper's memset); foreign[ 1 + s ], s < slots: some of them */
__global__ __launch_bounds__( 256 )
void k_frame_foreign_scan( const long long* __restrict__ index, const double* __restrict__ pos_xy, uint64_t entries, uint64_t samples, uint64_t width,
                           uint64_t height, uint32_t slots, unsigned long long* __restrict__ foreign )
{
    const uint64_t step = ( uint64_t )gridDim.x * 256u;
    for( uint64_t e = ( uint64_t )blockIdx.x * 256u + threadIdx.x; e < entries; e += step )
    {
        const double2 p = *( const double2* )( pos_xy + 2 * e );
        const int64_t home = index ? ( int64_t )index[ e / samples ] : ( int64_t )( e / samples );
        const int64_t t = acn_frame_target( p.x, p.y, width, height );
        if( t < 0 || t == home ) continue;
        const unsigned long long s = atomicAdd( &foreign[ 0 ], 1ull );
        if( s < slots ) foreign[ 1 + s ] = e;
    }
}

__device__ static void frame_apply_one( double* acc, const double* pos_xy, const double* clr, uint64_t e, int64_t t )
{
    double rec[ 6 ];
    for( int w = 0; w < 6; w++ ) rec[ w ] = acc[ 6 * t + w ];
    acn_frame_add( rec, pos_xy[ 2 * e ], pos_xy[ 2 * e + 1 ], clr + 3 * e );
    for( int w = 0; w < 6; w++ ) acc[ 6 * t + w ] = rec[ w ];
}

/* one lane */
__global__ void k_frame_foreign_apply( const long long* __restrict__ index, const double* __restrict__ pos_xy, const double* __restrict__ clr, uint64_t entries,
                                       uint64_t samples, uint64_t width, uint64_t height, uint32_t slots, const unsigned long long* __restrict__ foreign,
                                       double* __restrict__ acc )
{
    const unsigned long long m = foreign[ 0 ];
    if( m == 0 ) return;
    if( m <= slots )
    {
        unsigned long long last = 0;   /* the entry added last; entry 0 is never foreign twice: `first` lets it through once */
        bool first = true;
        for( unsigned long long done = 0; done < m; done++ )
        {
            unsigned long long best = ~0ull;
            for( unsigned long long s = 0; s < m; s++ )
            {
                const unsigned long long e = foreign[ 1 + s ];
                if( ( first || e > last ) && e < best ) best = e;
            }
            frame_apply_one( acc, pos_xy, clr, best, acn_frame_target( pos_xy[ 2 * best ], pos_xy[ 2 * best + 1 ], width, height ) );
            last = best; first = false;
        }
        return;
    }
    for( uint64_t e = 0; e < entries; e++ )
    {
        const int64_t home = index ? ( int64_t )index[ e / samples ] : ( int64_t )( e / samples );
        const int64_t t = acn_frame_target( pos_xy[ 2 * e ], pos_xy[ 2 * e + 1 ], width, height );
        if( t >= 0 && t != home ) frame_apply_one( acc, pos_xy, clr, e, t );
    }
}

/* groups [ g0, g0 + cnt ) of a plan */
__global__ __launch_bounds__( 256 )
void k_frame_push( const long long* __restrict__ index, const double* __restrict__ pos_xy, const double* __restrict__ clr, uint64_t g0, uint64_t cnt,
                   uint64_t samples, uint64_t width, uint64_t height, double* __restrict__ acc )
{
    const uint64_t t = ( uint64_t )blockIdx.x * 256u + threadIdx.x;
    if( t >= cnt ) return;
    const uint64_t r = g0 + t;
    const int64_t home = index ? ( int64_t )index[ r ] : ( int64_t )r;
    double2* a = ( double2* )( acc + 6 * home );
    const double2 a0 = a[ 0 ], a1 = a[ 1 ], a2 = a[ 2 ];
    double rec[ 6 ] = { a0.x, a0.y, a1.x, a1.y, a2.x, a2.y };
    for( uint64_t k = 0; k < samples; k++ )
    {
        const uint64_t e = r * samples + k;
        const double2 p = *( const double2* )( pos_xy + 2 * e );
        if( acn_frame_target( p.x, p.y, width, height ) != home ) continue;   /* foreign, or outside the raster */
        const double c[ 3 ] = { clr[ 3 * e ], clr[ 3 * e + 1 ], clr[ 3 * e + 2 ] };
        acn_frame_add( rec, p.x, p.y, c );
    }
    a[ 0 ] = make_double2( rec[ 0 ], rec[ 1 ] );
    a[ 1 ] = make_double2( rec[ 2 ], rec[ 3 ] );
    a[ 2 ] = make_double2( rec[ 4 ], rec[ 5 ] );
}

__global__ __launch_bounds__( 256 )
void k_frame_image( const double* __restrict__ acc, uint64_t pixels, double* __restrict__ out_rgb, unsigned char* __restrict__ out_rgb8 )
{
    const uint64_t p = ( uint64_t )blockIdx.x * 256u + threadIdx.x;
    if( p >= pixels ) return;
    const double2* r = ( const double2* )( acc + 6 * p );
    const double2 lo = r[ 1 ], hi = r[ 2 ];
    const double rec[ 6 ] = { 0.0, 0.0, lo.x, lo.y, hi.x, hi.y };
    double a[ 3 ];
    acn_frame_avg( rec, a );
    if( out_rgb ) { out_rgb[ 3 * p ] = a[ 0 ]; out_rgb[ 3 * p + 1 ] = a[ 1 ]; out_rgb[ 3 * p + 2 ] = a[ 2 ]; }
    if( out_rgb8 ) { out_rgb8[ 3 * p ] = acn_frame_cps( a[ 0 ] ); out_rgb8[ 3 * p + 1 ] = acn_frame_cps( a[ 1 ] ); out_rgb8[ 3 * p + 2 ] = acn_frame_cps( a[ 2 ] ); }
}

/* ------------------------------------------------------------------------------------------------------------------ */
static unsigned blocks_of( uint64_t n ) { return ( unsigned )( ( n + 255 ) / 256 ); }

void acn_launch_frame_key( const double* acc, uint64_t width, uint64_t height, double* key, hipStream_t stream )
{
    const uint64_t tiles_x = ( width + KEY_TW - 1 ) / KEY_TW, tiles_y = ( height + KEY_TH - 1 ) / KEY_TH;
    hipLaunchKernelGGL( k_frame_key, dim3( ( unsigned )( tiles_x * tiles_y ) ), dim3( 256 ), 0, stream, acc, ( uint32_t )width, ( uint32_t )height,
                        ( uint32_t )tiles_x, key );
}

void acn_launch_frame_jitter( const long long* index, uint64_t e0, uint64_t cnt, uint64_t samples, uint64_t rval, uint64_t width, double* pos_xy,
                              hipStream_t stream )
{
    hipLaunchKernelGGL( k_frame_jitter, dim3( blocks_of( cnt ) ), dim3( 256 ), 0, stream, index, e0, cnt, samples, rval, width, pos_xy );
}

void acn_launch_frame_foreign( const long long* index, const double* pos_xy, const double* clr, uint64_t entries, uint64_t samples, uint64_t width,
                               uint64_t height, uint32_t slots, unsigned long long* foreign, double* acc, hipStream_t stream )
{
    ( void )hipMemsetAsync( foreign, 0, sizeof( unsigned long long ), stream );
    uint64_t grid = ( entries + 2047 ) / 2048;   /* eight entries per lane before the grid is bounded */
    if( grid > 1024 ) grid = 1024;
    hipLaunchKernelGGL( k_frame_foreign_scan, dim3( ( unsigned )grid ), dim3( 256 ), 0, stream, index, pos_xy, entries, samples, width, height, slots, foreign );
    hipLaunchKernelGGL( k_frame_foreign_apply, dim3( 1 ), dim3( 1 ), 0, stream, index, pos_xy, clr, entries, samples, width, height, slots,
                        ( const unsigned long long* )foreign, acc );
}

void acn_launch_frame_push( const long long* index, const double* pos_xy, const double* clr, uint64_t g0, uint64_t cnt, uint64_t samples,
                            uint64_t width, uint64_t height, double* acc, hipStream_t stream )
{
    hipLaunchKernelGGL( k_frame_push, dim3( blocks_of( cnt ) ), dim3( 256 ), 0, stream, index, pos_xy, clr, g0, cnt, samples, width, height, acc );
}

void acn_launch_frame_image( const double* acc, uint64_t pixels, double* out_rgb, unsigned char* out_rgb8, hipStream_t stream )
{
    hipLaunchKernelGGL( k_frame_image, dim3( blocks_of( pixels ) ), dim3( 256 ), 0, stream, acc, pixels, out_rgb, out_rgb8 );
}
