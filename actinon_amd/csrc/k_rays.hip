/* k_rays.hip -- caller-supplied primary rays (acn_render_rays, acn_camera_rays; include/actinon_hip.h).
 *
 * In the reference radiance is a function of a ray: lum_machine_s_func (src/scene.c:956-1013) builds a pinhole ray and hands
 * it to scene_s_trans_hit + scene_s_lum.  A ray call enters the pipeline where k_walk already reads rays in every pass but
 * pass 0 of level 0: k_seed_rays fills generation 0 of level 0 with the caller's rays, and the host launches that pass with
 * no camera rays (n_cam = 0).  Everything after is the production chain, untouched.  A seed carries what k_walk gives a
 * camera ray (acn_k_walk.h, k_walk: T = 1, intensity = 1, depth = trace_depth, the slot's position as its pixel), so a
 * camera ray handed in as a caller's ray is traced and shaded exactly as the pipeline's own. */
#include <hip/hip_runtime.h>
#include "acn_device.h"   /* a ray unit: the whole tracer */
#include "acn_launch.h"

__global__ void k_seed_rays( const double* __restrict__ rays, uint32_t base, uint32_t cnt, TileOrder order, int depth,
                             RayTask* __restrict__ out, uint32_t* __restrict__ gen0 )
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if( i == 0 ) *gen0 = cnt;
    if( i >= cnt ) return;
    const uint32_t p = order.position( base + i );
    RayTask r;
    r.T = mk( 1, 1, 1 ); r.intensity = 1.0; r.depth = depth;
    if( p < order.n )
    {
        const double* src = rays + ( size_t )p * 6;
        r.p = ld3( src );
        r.d = v_of_length( ld3( src + 3 ), 1.0 );   /* vectors.h:148-154: unchanged, bit for bit, when | |d|^2 - 1 | < 1e-8 */
        r.pixel = p;
    }
    else   /* (slots past the call's last ray: the last tile of the order is short, or a learning sample's stride overshoots) */
    {
        r.p = mk( 0, 0, 0 ); r.d = mk( 0, 0, 1 ); r.pixel = ACN_INVALID;
    }
    out[ i ] = r;
}

__global__ void k_check_rays( const double* __restrict__ rays, size_t n, unsigned long long* __restrict__ first_bad )
{
    const size_t i = ( size_t )blockIdx.x * blockDim.x + threadIdx.x;
    if( i >= n ) return;
    const double* r = rays + i * 6;
    bool ok = true;
    for( int k = 0; k < 6; k++ ) ok = ok && __builtin_isfinite( r[ k ] );
    /* v_of_length scales by 1 / sqrt( |d|^2 ): a square that is 0 (a zero direction, or one that underflows) or that
     * overflows would leave a zero direction */
    const double sq = v_sqr( ld3( r + 3 ) );
    ok = ok && sq > 0.0 && sq < F3_INF;
    if( !ok ) atomicMin( first_bad, ( unsigned long long )i );
}

__global__ void k_camera_rays( DevScene sc, const double* __restrict__ pos_xy, size_t n, double* __restrict__ out )
{
    const size_t i = ( size_t )blockIdx.x * blockDim.x + threadIdx.x;
    if( i >= n ) return;
    V3 rp, rd;
    camera_ray( sc, pos_xy[ i * 2 ], pos_xy[ i * 2 + 1 ], &rp, &rd );
    double* o = out + i * 6;
    o[ 0 ] = rp.x; o[ 1 ] = rp.y; o[ 2 ] = rp.z;
    o[ 3 ] = rd.x; o[ 4 ] = rd.y; o[ 5 ] = rd.z;
}

void acn_launch_seed_rays( const double* rays, uint32_t base, uint32_t cnt, TileOrder order, int depth, const LevelQ& q, hipStream_t stream )
{
    const uint32_t n = cnt < q.ray_cap ? cnt : q.ray_cap;
    hipLaunchKernelGGL( k_seed_rays, dim3( ( n + 255 ) / 256 ), dim3( 256 ), 0, stream, rays, base, n, order, depth, q.rays[ 0 ], q.counts + QC_GEN );
}

void acn_launch_check_rays( const double* rays, size_t n, unsigned long long* first_bad, hipStream_t stream )
{
    hipLaunchKernelGGL( k_check_rays, dim3( ( unsigned )( ( n + 255 ) / 256 ) ), dim3( 256 ), 0, stream, rays, n, first_bad );
}

void acn_launch_camera_rays( const DevScene& sc, const double* pos_xy, size_t n, double* out, hipStream_t stream )
{
    hipLaunchKernelGGL( k_camera_rays, dim3( ( unsigned )( ( n + 255 ) / 256 ) ), dim3( 256 ), 0, stream, sc, pos_xy, n, out );
}
