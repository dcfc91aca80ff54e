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
 *                  split, so a result does not depend on which positions share a wavefront or a workgroup. */
#include <hip/hip_runtime.h>
#include "acn_launch.h"

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
        for( uint32_t idx = tid; idx < np * row; idx += 256 )
        {
            const uint32_t p = idx / row, r = idx - p * row;
            tile[ idx ] = rad[ ( ( p0 + p ) * K + k0 ) * 3 + r ];
        }
        __syncthreads();
        if( adds ) for( uint32_t k = 0; k < kc; k++ ) sum = sum + tile[ my_p * row + k * 3 + my_c ];
        __syncthreads();
    }
    if( !adds ) return;
    double mean = sum / ( double )K;
    if( !linear ) mean = cl_sat( mk( mean, mean, mean ), gamma ).x;   /* (per channel: a power and a clamp) */
    out_rgb[ p0 * 3 + tid ] = mean;
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
