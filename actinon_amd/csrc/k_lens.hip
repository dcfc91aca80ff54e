/* k_lens.hip -- the thin-lens camera of acn_lens_rays / acn_render_lens (include/actinon_hip.h states every expression and its
 * order; tests/lens_model.py restates them in numpy and the two are compared bit for bit).
 *
 * The reference has a pinhole only (camera_ray, src/scene.c:980-990); the lens is a definition of this library.  A lens call makes
 * K primary rays per sample position, hands them to the production pipeline as a ray call (k_rays.hip: seeded generation 0) and
 * averages the K radiances of a position in the order of k.
 *   k_lens_rays    one (position, sample) per lane.  Every draw comes from the lane's own LCG state, seeded from the position and
 *                  the sample number: a ray depends on nothing but ( px, py, k ) and the call's parameters.
 *   k_lens_reduce  radiance is [ position ][ k ][ 3 ]: the K * 3 doubles of a position are contiguous, so a lane that walked its
 *                  position's samples alone would stride K * 24 bytes from its neighbour.  A workgroup therefore takes
 *                  LENS_TILE_POS consecutive positions and copies LENS_TILE_K samples of each at a time into LDS with consecutive
 *                  lanes on consecutive doubles (the whole tile is one contiguous run when K <= LENS_TILE_K, else runs of
 *                  LENS_TILE_K * 24 bytes), and lane t < 3 * positions then adds channel t % 3 of position t / 3 from LDS, alone
 *                  and in the order of k: ( ( 0.0 + L0 ) + L1 ) + ...  No lane reads another lane's registers and no sum is
 *                  split, so a result does not depend on which positions share a wavefront or a workgroup.
 *                  lens_stage copies a tile, for this kernel and both passes of the next.
 *   k_lens_reduce_stats  k_lens_reduce with the record of every position, behind acn_render_lens_stats*: pass 1 is that sum, pass 2
 *                  stages the tiles again (not when K <= LENS_TILE_K: the one tile is still in LDS) and the same lane adds the
 *                  squared deviations from its mean in the order of k.  The 64-byte records of the workgroup are put together in
 *                  LDS and leave as 16-byte pieces, consecutive lanes on consecutive pieces: 64 positions are one run of 4 KiB.
 *   k_stats_merge, k_stats_resolve  one record per lane, read and written as four 16-byte pieces; the record's rules (EMPTY, the
 *                  variance of the mean) are those of acn_stats_dev.h, which the filters read too. */
#include <hip/hip_runtime.h>
#include "acn_launch.h"
#include "acn_stats_dev.h"

#define LENS_TILE_POS 64
#define LENS_TILE_K   16
#define LENS_ROUNDS   32   /* rejection rounds of the disc sample */

__global__ __launch_bounds__( 256 )
void k_lens_rays( DevScene sc, const double* __restrict__ pos_xy, size_t first_pixel, size_t n, LensSetup ls,
                  uint32_t first_sample, uint32_t n_samples, double* __restrict__ out )
{
    const size_t t = ( size_t )blockIdx.x * blockDim.x + threadIdx.x;
    if( t >= n * n_samples ) return;
    const size_t i = t / n_samples;
    const uint32_t k = first_sample + ( uint32_t )( t - i * n_samples );
    double px, py;
    if( pos_xy ) { px = pos_xy[ i * 2 ]; py = pos_xy[ i * 2 + 1 ]; }
    else   /* the pixel centres of acn_render_main_pass_dev */
    {
        const size_t pix = first_pixel + i;
        px = ( double )( pix % sc.prm.image_width ) + 0.5;
        py = ( double )( pix / sc.prm.image_width ) + 0.5;
    }
    /* (2 k + 1, not k + 1: v_random_seed reads only the frexp mantissa of a component, which k + 1 = 1, 2, 4, 8 ... would share) */
    uint64_t rv = v_random_seed( mk( px, py, ( double )( 2 * k + 1 ) ), ls.seed );
    double qx = px, qy = py;
    if( ls.jitter )
    {
        const double jx = f3_rnd1( &rv ) - 0.5;
        const double jy = f3_rnd1( &rv ) - 0.5;
        qx = px + jx; qy = py + jy;
    }
    V3 o, d;
    camera_ray( sc, qx, qy, &o, &d );
    if( ls.aperture_radius != 0.0 )
    {
        double u = 0.0, v = 0.0;
        for( int round = 0; round < LENS_ROUNDS; round++ )
        {
            const double a = f3_rnd0( &rv );
            const double b = f3_rnd0( &rv );
            if( a * a + b * b <= 1.0 ) { u = a; v = b; break; }
        }
        const V3 R = m_mlv( sc.camera_rotation, mk( 1, 0, 0 ) );
        const V3 V = m_mlv( sc.camera_rotation, mk( 0, 1, 0 ) );
        const V3 T = m_mlv( sc.camera_rotation, mk( 0, 0, 1 ) );
        const double ft = ls.focus_distance / v_mlv( d, V );
        const V3 F = v_add( o, v_mlf( d, ft ) );
        o = v_add( o, v_add( v_mlf( R, ls.aperture_radius * u ), v_mlf( T, ls.aperture_radius * v ) ) );
        d = v_of_length( v_sub( F, o ), 1.0 );
    }
    double* r = out + t * 6;
    r[ 0 ] = o.x; r[ 1 ] = o.y; r[ 2 ] = o.z;
    r[ 3 ] = d.x; r[ 4 ] = d.y; r[ 5 ] = d.z;
}

/* samples [ k0, k0 + row / 3 ) of the workgroup's positions [ p0, p0 + np ) -> LDS, consecutive lanes on consecutive doubles.  The
 * barriers around it are the caller's */
__device__ static inline void lens_stage( double* tile, const double* __restrict__ rad, size_t p0, uint32_t np, uint32_t K, uint32_t k0, uint32_t row )
{
    for( uint32_t idx = threadIdx.x; idx < np * row; idx += 256 )
    {
        const uint32_t p = idx / row, r = idx - p * row;
        tile[ idx ] = rad[ ( ( p0 + p ) * K + k0 ) * 3 + r ];
    }
}

__global__ __launch_bounds__( 256 )
void k_lens_reduce( const double* __restrict__ rad, size_t n, uint32_t K, double gamma, int linear, double* __restrict__ out_rgb )
{
    __shared__ double tile[ LENS_TILE_POS * LENS_TILE_K * 3 ];
    const size_t p0 = ( size_t )blockIdx.x * LENS_TILE_POS;
    const uint32_t np = n - p0 < LENS_TILE_POS ? ( uint32_t )( n - p0 ) : LENS_TILE_POS;
    const uint32_t tid = threadIdx.x;
    const bool adds = tid < np * 3;
    const uint32_t my_p = tid / 3, my_c = tid - my_p * 3;
    double sum = 0.0;
    for( uint32_t k0 = 0; k0 < K; k0 += LENS_TILE_K )
    {
        const uint32_t kc = K - k0 < LENS_TILE_K ? K - k0 : LENS_TILE_K, row = kc * 3;
        lens_stage( tile, rad, p0, np, K, k0, row );
        __syncthreads();
        if( adds ) for( uint32_t k = 0; k < kc; k++ ) sum = sum + tile[ my_p * row + k * 3 + my_c ];
        __syncthreads();
    }
    if( !adds ) return;
    double mean = sum / ( double )K;
    if( !linear ) mean = cl_sat( mk( mean, mean, mean ), gamma ).x;   /* (per channel: a power and a clamp) */
    out_rgb[ p0 * 3 + tid ] = mean;
}

/* k_lens_reduce plus the record of every position (include/actinon_hip.h, ACN_STATS_STRIDE): n = K, the mean, and
 * m2 = ( ( 0.0 + d0 * d0 ) + d1 * d1 ) + ..., dk = Lk - mean, a second pass over the samples.  out_rgb may be null */
__global__ __launch_bounds__( 256 )
void k_lens_reduce_stats( const double* __restrict__ rad, size_t n, uint32_t K, double gamma, int linear, double* __restrict__ out_rgb,
                          double2* __restrict__ stats )
{
    __shared__ double tile[ LENS_TILE_POS * LENS_TILE_K * 3 ];
    __shared__ double2 rec[ LENS_TILE_POS * 4 ];
    const size_t p0 = ( size_t )blockIdx.x * LENS_TILE_POS;
    const uint32_t np = n - p0 < LENS_TILE_POS ? ( uint32_t )( n - p0 ) : LENS_TILE_POS;
    const uint32_t tid = threadIdx.x;
    const bool adds = tid < np * 3;
    const uint32_t my_p = tid / 3, my_c = tid - my_p * 3;
    double sum = 0.0;
    for( uint32_t k0 = 0; k0 < K; k0 += LENS_TILE_K )
    {
        const uint32_t kc = K - k0 < LENS_TILE_K ? K - k0 : LENS_TILE_K, row = kc * 3;
        if( k0 ) __syncthreads();   /* (the adds of the tile before) */
        lens_stage( tile, rad, p0, np, K, k0, row );
        __syncthreads();
        if( adds ) for( uint32_t k = 0; k < kc; k++ ) sum = sum + tile[ my_p * row + k * 3 + my_c ];
    }
    const double mean = sum / ( double )K;
    double m2 = 0.0;
    for( uint32_t k0 = 0; k0 < K; k0 += LENS_TILE_K )
    {
        const uint32_t kc = K - k0 < LENS_TILE_K ? K - k0 : LENS_TILE_K, row = kc * 3;
        if( K > LENS_TILE_K )   /* else the one tile of pass 1 is still there */
        {
            __syncthreads();
            lens_stage( tile, rad, p0, np, K, k0, row );
            __syncthreads();
        }
        if( adds ) for( uint32_t k = 0; k < kc; k++ )
        {
            const double d = tile[ my_p * row + k * 3 + my_c ] - mean;
            m2 = m2 + d * d;
        }
    }
    if( adds )
    {
        double* r = ( double* )rec + my_p * ACN_STATS_STRIDE;
        r[ 1 + my_c ] = mean;
        r[ 4 + my_c ] = m2;
        if( my_c == 0 ) { r[ 0 ] = ( double )K; r[ 7 ] = 0.0; }
        if( out_rgb ) out_rgb[ p0 * 3 + tid ] = linear ? mean : cl_sat( mk( mean, mean, mean ), gamma ).x;   /* (as k_lens_reduce) */
    }
    __syncthreads();
    if( tid < np * 4 ) stats[ p0 * 4 + tid ] = rec[ tid ];
}

/* acc[ i ] <- merge( acc[ i ], part[ j ] ), i = index ? index[ j ] : j; an i outside [ 0, n_acc ) is skipped: nothing is read or written */
__global__ __launch_bounds__( 256 )
void k_stats_merge( double2* acc, size_t n_acc, const double2* __restrict__ part, size_t n_part, const long long* __restrict__ index )
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
    StatsRec rb;
    rb.q[ 0 ] = part[ 4 * j ]; rb.q[ 1 ] = part[ 4 * j + 1 ]; rb.q[ 2 ] = part[ 4 * j + 2 ]; rb.q[ 3 ] = part[ 4 * j + 3 ];
    if( stats_empty( rb.q[ 0 ].x ) ) return;
    double2* a = acc + 4 * ( size_t )i;
    StatsRec ra;
    ra.q[ 0 ] = a[ 0 ]; ra.q[ 1 ] = a[ 1 ]; ra.q[ 2 ] = a[ 2 ]; ra.q[ 3 ] = a[ 3 ];
    const StatsRec r = stats_empty( ra.q[ 0 ].x ) ? rb : stats_pair_merge( ra, rb );   /* (an EMPTY a: b, bit for bit) */
    a[ 0 ] = r.q[ 0 ]; a[ 1 ] = r.q[ 1 ]; a[ 2 ] = r.q[ 2 ]; a[ 3 ] = r.q[ 3 ];
}

/* out_rgb (nullable): the mean, or the background of an EMPTY record, through cl_s_sat unless linear; out_noise (nullable): `noise` */
__global__ __launch_bounds__( 256 )
void k_stats_resolve( const double2* __restrict__ stats, size_t n, double bg_x, double bg_y, double bg_z, double gamma, int linear,
                      double* __restrict__ out_rgb, double* __restrict__ out_noise )
{
    const size_t i = ( size_t )blockIdx.x * blockDim.x + threadIdx.x;
    if( i >= n ) return;
    StatsRec r;
    r.q[ 0 ] = stats[ 4 * i ]; r.q[ 1 ] = stats[ 4 * i + 1 ]; r.q[ 2 ] = stats[ 4 * i + 2 ]; r.q[ 3 ] = stats[ 4 * i + 3 ];
    stats_resolve_write( r, i, bg_x, bg_y, bg_z, gamma, linear, out_rgb, out_noise );
}

void acn_launch_lens_rays( const DevScene& sc, const double* pos_xy, size_t first_pixel, size_t n, const LensSetup& ls,
                           uint32_t first_sample, uint32_t n_samples, double* out_rays, hipStream_t stream )
{
    const size_t items = n * n_samples;
    hipLaunchKernelGGL( k_lens_rays, dim3( ( unsigned )( ( items + 255 ) / 256 ) ), dim3( 256 ), 0, stream,
                        sc, pos_xy, first_pixel, n, ls, first_sample, n_samples, out_rays );
}

void acn_launch_lens_reduce( const double* rad, size_t n, uint32_t samples, double gamma, int linear, double* out_rgb, hipStream_t stream )
{
    hipLaunchKernelGGL( k_lens_reduce, dim3( ( unsigned )( ( n + LENS_TILE_POS - 1 ) / LENS_TILE_POS ) ), dim3( 256 ), 0, stream,
                        rad, n, samples, gamma, linear, out_rgb );
}

void acn_launch_lens_reduce_stats( const double* rad, size_t n, uint32_t samples, double gamma, int linear, double* out_rgb, double* stats,
                                   hipStream_t stream )
{
    hipLaunchKernelGGL( k_lens_reduce_stats, dim3( ( unsigned )( ( n + LENS_TILE_POS - 1 ) / LENS_TILE_POS ) ), dim3( 256 ), 0, stream,
                        rad, n, samples, gamma, linear, out_rgb, ( double2* )stats );
}

void acn_launch_stats_merge( double* acc, size_t n_acc, const double* part, size_t n_part, const int64_t* index, hipStream_t stream )
{
    hipLaunchKernelGGL( k_stats_merge, dim3( ( unsigned )( ( n_part + 255 ) / 256 ) ), dim3( 256 ), 0, stream,
                        ( double2* )acc, n_acc, ( const double2* )part, n_part, ( const long long* )index );
}

void acn_launch_stats_resolve( const double* stats, size_t n, const double* background, double gamma, int linear, double* out_rgb,
                               double* out_noise, hipStream_t stream )
{
    hipLaunchKernelGGL( k_stats_resolve, dim3( ( unsigned )( ( n + 255 ) / 256 ) ), dim3( 256 ), 0, stream,
                        ( const double2* )stats, n, background[ 0 ], background[ 1 ], background[ 2 ], gamma, linear, out_rgb, out_noise );
}
