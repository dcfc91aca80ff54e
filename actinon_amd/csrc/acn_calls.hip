/* acn_calls.hip -- the entry points of include/actinon_hip.h that stand beside the pipeline: camera rays, surface records, resolve,
 * denoise, the thin-lens camera, its sample statistics and the fill of a sparse frame of them, its surface records and its layered records, select and key histogram, projection and reprojection (with the motion table), shadow records and the history guard, the device-resident frame, and the two test seams acn_estimate_envelope
 * and acn_detmath_eval with the kernels only they launch.  Each is a frame (Call, acn_handle.h) around launch wrappers of
 * acn_launch.h; what renders goes through render_dispatch of actinon_hip.hip, which holds the pipeline and its own entry points.
 * The lens calls that cut their positions into slices share one loop, lens_slices; a host-buffer form is a HostCall (acn_handle.h). */
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>

#include "acn_device.h"   /* a ray unit: the whole tracer */
#include "acn_handle.h"
#include "acn_stats_host.h"
#include "acn_fill_host.h"
#include "acn_select_host.h"
#include "acn_lenssurf_host.h"
#include "acn_layers_host.h"
#include "acn_reproject_host.h"
#include "acn_motion_host.h"
#include "acn_shadow_host.h"

/* ------------------------------------------------------------------------------------------------------------------ */
/* kernels */

/* cl_s_sat + cps_from_cl after the (cross-GPU) accumulation */
__global__ void k_resolve( const double* __restrict__ lin, size_t n, double gamma, double* __restrict__ out_rgb,
                           unsigned char* __restrict__ out_rgb8 )
{
    size_t i = ( size_t )blockIdx.x * blockDim.x + threadIdx.x;
    if( i >= n ) return;
    V3 c = cl_sat( mk( lin[ i * 3 ], lin[ i * 3 + 1 ], lin[ i * 3 + 2 ] ), gamma );
    if( out_rgb ) { out_rgb[ i * 3 ] = c.x; out_rgb[ i * 3 + 1 ] = c.y; out_rgb[ i * 3 + 2 ] = c.z; }
    if( out_rgb8 )
    {
        out_rgb8[ i * 3 + 0 ] = c.x > 0.0 ? c.x < 1.0 ? ( unsigned char )( c.x * 256 ) : 255 : 0;
        out_rgb8[ i * 3 + 1 ] = c.y > 0.0 ? c.y < 1.0 ? ( unsigned char )( c.y * 256 ) : 255 : 0;
        out_rgb8[ i * 3 + 2 ] = c.z > 0.0 ? c.z < 1.0 ? ( unsigned char )( c.z * 256 ) : 255 : 0;
    }
}

/* obj_ray_exit + obj_estimate_envelope (objects.c:286-363), one lane */
__global__ void k_estimate_envelope( DevScene sc, int node, uint64_t samples, uint32_t rseed, double radius_factor,
                                     V3* scratch, double* out )
{
    Cnt< false > cnt;
    NodeP hdr = &sc.nodes[ node ];
    uint64_t size = 0;
    V3 sum = mk( 0, 0, 0 );
    uint64_t rv = rseed;
    V3 rp = ld3( hdr->pos );
    for( uint64_t i = 0; i < samples; i++ )
    {
        V3 rd = v_random_sphere_belt( &rv, 1.0 );
        /* obj_ray_exit */
        double exit_a = F3_INF;
        {
            V3 nor = mk( 0, 0, 0 );
            double a = obj_ray_hit_dev( sref( sc ), node, rp, rd, true, &nor, &cnt );
            if( a < F3_INF )
            {
                V3 lp = rp;
                double s = 0;
                while( a < F3_INF )
                {
                    a += F3_EPS * 2;
                    s += a;
                    lp = ray_pos( lp, rd, a );
                    a = obj_ray_hit_dev( sref( sc ), node, lp, rd, true, &nor, &cnt );
                }
                if( v_mlv( nor, rd ) > 0 ) exit_a = s;
            }
        }
        if( exit_a < F3_INF )
        {
            V3 pos = ray_pos( rp, rd, exit_a );
            scratch[ size++ ] = pos;
            sum = v_add( sum, ray_pos( rp, rd, exit_a ) );
            rp = v_mlf( sum, ( 1.0 / size ) );
            rp.x += F3_EPS * f3_rnd0( &rv );
            rp.y += F3_EPS * f3_rnd0( &rv );
            rp.z += F3_EPS * f3_rnd0( &rv );
        }
    }
    double radius = F3_MAG;
    if( size > 0 )
    {
        double max_r2 = 0;
        for( uint64_t i = 0; i < size; i++ )
        {
            double r = v_diff_sqr( rp, scratch[ i ] );
            max_r2 = r > max_r2 ? r : max_r2;
        }
        radius = acn_sqrt( max_r2 ) * radius_factor;
    }
    out[ 0 ] = rp.x; out[ 1 ] = rp.y; out[ 2 ] = rp.z; out[ 3 ] = radius;
}

__global__ void k_detmath( int op, const double* x, const double* y, double* out, size_t n )
{
    size_t i = ( size_t )blockIdx.x * blockDim.x + threadIdx.x;
    if( i >= n ) return;
    double a = x[ i ], b = y ? y[ i ] : 0.0, r = 0;
    switch( op )
    {
        case 0: r = acn_sin( a ); break;
        case 1: r = acn_cos( a ); break;
        case 2: r = acn_tan( a ); break;
        case 3: r = acn_acos( a ); break;
        case 4: r = acn_log( a ); break;
        case 5: r = acn_exp( a ); break;
        case 6: r = acn_pow( a, b ); break;
        case 7: r = acn_sqrt( a ); break;
        case 8: r = a / b; break;
        case 9: r = ( double )acn_f64_bits( a ); break;
        case 10: r = acn_frexp_mant( a ); break;
        case 11: r = acn_asin( a ); break;
        case 12: r = acn_atan( a ); break;
        case 13: r = acn_atan2( a, b ); break;
        case 14: r = ( double )acn_llrint( a ); break;   /* |a| < 2^62 (the conversion is undefined beyond long long) */
        default: break;
    }
    out[ i ] = r;
}

/* ------------------------------------------------------------------------------------------------------------------ */
/* ABI */
extern "C" int acn_camera_rays_dev( acn_scene_handle* h, const void* d_pos_xy, size_t n, void* d_out_rays, const acn_render_opts* opts )
{
    Call c( opts );
    if( !h || ( n && ( !d_pos_xy || !d_out_rays ) ) ) return fail( ACN_ERR_ARG, "null argument" );
    if( n == 0 ) return ACN_OK;
    if( n > 0xFFFFFF00ull ) return fail( ACN_ERR_ARG, "too many positions in one call" );
    int st = call_begin( h, &c );
    if( st != ACN_OK ) return st;
    acn_launch_camera_rays( h->dev, ( const double* )d_pos_xy, n, ( double* )d_out_rays, c.stream );
    HIP_TRY( hipGetLastError() );
    return call_end( c );
}

extern "C" int acn_camera_rays( acn_scene_handle* h, const double* pos_xy, size_t n, double* out_rays )
{
    if( !h || ( n && ( !pos_xy || !out_rays ) ) ) return fail( ACN_ERR_ARG, "null argument" );
    if( n == 0 ) return ACN_OK;
    return host_in_out( h, pos_xy, sizeof( double ) * 2 * n, out_rays, sizeof( double ) * 6 * n,
                        [ & ]( void* d_pos, void* d_out ) { return acn_camera_rays_dev( h, d_pos, n, d_out, nullptr ); } );
}

/* ---- surface records (k_surface.hip) ---- */
/* the word that takes ACN_FLAG_STACK_OVERFLOW of the surface kernels (the pipeline's word stays the pipeline's): made on first use */
static int surface_flags_begin( acn_scene_handle* h, SceneArgs* s )
{
    if( !h->d_surface_flags.get() )
    {
        if( h->d_surface_flags.grow( sizeof( uint32_t ) ) ) return ACN_ERR_DEVICE;
        HIP_TRY( hipMemset( h->d_surface_flags.get(), 0, sizeof( uint32_t ) ) );
    }
    *s = scene_args( h->dev, h->scene );
    s->dev.flags = h->d_surface_flags.get();
    return ACN_OK;
}

/* the end of a call that launched surface kernels: on the handle's own stream the call waits and reads the word; a caller's stream is
 * not synchronised for it */
static int surface_flags_end( acn_scene_handle* h, const Call& c )
{
    if( !c.own ) return ACN_OK;
    uint32_t flags = 0;
    HIP_TRY( hipMemcpyAsync( &flags, h->d_surface_flags.get(), sizeof( flags ), hipMemcpyDeviceToHost, c.stream ) );
    int st = call_end( c );
    if( st != ACN_OK ) return st;
    if( flags )
    {
        HIP_TRY( hipMemset( h->d_surface_flags.get(), 0, sizeof( uint32_t ) ) );
        return fail( ACN_ERR_UNSUPPORTED, "device CSG / compound stack overflow in a surface call" );
    }
    return ACN_OK;
}

static int surface_mode_check( uint32_t mode, const acn_render_opts& opts )
{
    if( mode != ACN_SURF_FIRST_HIT && mode != ACN_SURF_FOLLOW ) return fail( ACN_ERR_ARG, "unknown surface mode " + std::to_string( mode ) );
    if( opts.shard_world > 1 ) return fail( ACN_ERR_ARG, "a surface call is not sharded: slice the array" );
    return ACN_OK;
}

static int surface_dev( acn_scene_handle* h, const double* d_rays, const double* d_pos_xy, size_t n, uint32_t mode, double* d_out, Call& c )
{
    if( !h || ( n && ( !( d_rays || d_pos_xy ) || !d_out ) ) ) return fail( ACN_ERR_ARG, "null argument" );
    int st = surface_mode_check( mode, c.opts );
    if( st != ACN_OK || n == 0 ) return st;
    if( ( st = call_begin( h, &c ) ) != ACN_OK ) return st;
    SceneArgs s;
    if( ( st = surface_flags_begin( h, &s ) ) != ACN_OK ) return st;
    if( d_rays && ( st = check_rays( h, d_rays, n, c.stream ) ) != ACN_OK ) return st;
    acn_launch_surface( mode, h->scene.lds_bytes != 0, machine_lds_bytes( h->scene ), c.stream, s, d_rays, d_pos_xy, n, d_out );
    HIP_TRY( hipGetLastError() );
    return surface_flags_end( h, c );
}

extern "C" int acn_surface_rays_dev( acn_scene_handle* h, const void* d_rays, size_t n, uint32_t mode, void* d_out, const acn_render_opts* opts )
{
    Call c( opts );
    if( !h || ( n && !d_rays ) ) return fail( ACN_ERR_ARG, "null argument" );
    return surface_dev( h, ( const double* )d_rays, nullptr, n, mode, ( double* )d_out, c );
}

extern "C" int acn_surface_positions_dev( acn_scene_handle* h, const void* d_pos_xy, size_t n, uint32_t mode, void* d_out, const acn_render_opts* opts )
{
    Call c( opts );
    if( !h || ( n && !d_pos_xy ) ) return fail( ACN_ERR_ARG, "null argument" );
    return surface_dev( h, nullptr, ( const double* )d_pos_xy, n, mode, ( double* )d_out, c );
}

/* the host-buffer forms: synchronous, on the handle's own stream */
static int surface_host( acn_scene_handle* h, const double* in, size_t in_len, size_t n, uint32_t mode, double* out, const acn_render_opts* opts )
{
    Call c( opts );
    if( !h || ( n && ( !in || !out ) ) ) return fail( ACN_ERR_ARG, "null argument" );
    const int st = surface_mode_check( mode, c.opts );
    if( st != ACN_OK || n == 0 ) return st;
    c.opts.stream = nullptr;
    return host_in_out( h, in, sizeof( double ) * in_len * n, out, sizeof( double ) * ACN_SURF_STRIDE * n, [ & ]( void* d_in, void* d_out )
    {
        return surface_dev( h, in_len == 6 ? ( const double* )d_in : nullptr, in_len == 6 ? nullptr : ( const double* )d_in, n, mode, ( double* )d_out, c );
    } );
}

extern "C" int acn_surface_rays( acn_scene_handle* h, const double* rays, size_t n, uint32_t mode, double* out, const acn_render_opts* opts )
{
    return surface_host( h, rays, 6, n, mode, out, opts );
}

extern "C" int acn_surface_positions( acn_scene_handle* h, const double* pos_xy, size_t n, uint32_t mode, double* out, const acn_render_opts* opts )
{
    return surface_host( h, pos_xy, 2, n, mode, out, opts );
}

extern "C" int acn_resolve_dev( acn_scene_handle* h, const void* d_linear_rgb, size_t n, void* d_out_rgb, void* d_out_rgb8,
                                const acn_render_opts* opts )
{
    Call c( opts );
    if( !h || ( n && !d_linear_rgb ) ) return fail( ACN_ERR_ARG, "null argument" );
    if( n == 0 ) return ACN_OK;
    int st = call_begin( h, &c );
    if( st != ACN_OK ) return st;
    hipLaunchKernelGGL( k_resolve, dim3( ( unsigned )( ( n + 255 ) / 256 ) ), dim3( 256 ), 0, c.stream,
                        ( const double* )d_linear_rgb, n, h->dev.prm.gamma, ( double* )d_out_rgb, ( unsigned char* )d_out_rgb8 );
    HIP_TRY( hipGetLastError() );
    return call_end( c );
}

/* ---- the edge-avoiding filter (k_denoise.hip) ---- */
struct DenoiseSetup { uint32_t iterations, normal_power_log2, no_demodulate; double sigma_plane, sigma_lum; };

/* every check of a denoise call: on the host, before the handle is touched */
static int denoise_check( const acn_scene_handle* h, const void* lin, const void* surf, size_t width, size_t height,
                          const acn_denoise_params* prm, const void* out, const acn_render_opts& opts, DenoiseSetup* su )
{
    if( !h || !lin || !surf || !out ) return fail( ACN_ERR_ARG, "null argument" );
    const size_t max_n = ( size_t )1 << 31;
    if( width == 0 || height == 0 ) return fail( ACN_ERR_ARG, "a frame to denoise needs a width and a height" );
    if( width > max_n || height > max_n || width * height > max_n ) return fail( ACN_ERR_ARG, "a frame to denoise has at most 2^31 pixels" );
    acn_denoise_params p{};
    if( prm )
    {
        if( prm->struct_size < sizeof( uint32_t ) ) return fail( ACN_ERR_ARG, "acn_denoise_params.struct_size " + std::to_string( prm->struct_size ) + " is smaller than its first member" );
        memcpy( &p, prm, prm->struct_size < sizeof( p ) ? prm->struct_size : sizeof( p ) );
    }
    if( p.flags & ~( ACN_DENOISE_NO_DEMODULATE | ACN_DENOISE_NORMAL_POWER_SET ) ) return fail( ACN_ERR_ARG, "unknown acn_denoise_params.flags bits" );
    if( p.iterations > ACN_DENOISE_MAX_ITERATIONS ) return fail( ACN_ERR_ARG, "acn_denoise_params.iterations " + std::to_string( p.iterations ) + " is above 8" );
    if( p.normal_power_log2 > ACN_DENOISE_MAX_NORMAL_POWER_LOG2 ) return fail( ACN_ERR_ARG, "acn_denoise_params.normal_power_log2 " + std::to_string( p.normal_power_log2 ) + " is above 10" );
    const double sig[ 2 ] = { p.sigma_plane, p.sigma_lum };
    for( double s : sig ) if( !( s >= 0 ) || s > 1.7976931348623157e308 ) return fail( ACN_ERR_ARG, "a sigma of acn_denoise_params is negative or not finite" );
    if( opts.shard_world > 1 ) return fail( ACN_ERR_ARG, "a denoise call is not sharded: the filter needs the whole frame" );
    su->iterations = p.iterations ? p.iterations : ACN_DENOISE_DEFAULT_ITERATIONS;
    su->normal_power_log2 = ( p.normal_power_log2 || ( p.flags & ACN_DENOISE_NORMAL_POWER_SET ) ) ? p.normal_power_log2 : ACN_DENOISE_DEFAULT_NORMAL_POWER_LOG2;
    su->no_demodulate = ( p.flags & ACN_DENOISE_NO_DEMODULATE ) ? 1u : 0u;
    su->sigma_plane = p.sigma_plane != 0 ? p.sigma_plane : ACN_DENOISE_DEFAULT_SIGMA_PLANE;
    su->sigma_lum = p.sigma_lum != 0 ? p.sigma_lum : ACN_DENOISE_DEFAULT_SIGMA_LUM;
    return ACN_OK;
}

/* ---- lens sample statistics: the checks that need no handle (acn_stats_host.h) ---- */
static int stats_buffer( const void* stats, size_t n, const char* what )
{
    std::string msg;
    return acn_stats_buffer_check( stats, n, what, &msg ) == ACN_OK ? ACN_OK : fail( ACN_ERR_ARG, msg );
}

/* acn_denoise_dev, and acn_denoise_stats_dev (from_stats): d_in is the linear frame, or the statistics records the filter takes
 * its colour and variance from */
static int denoise_dev( acn_scene_handle* h, const void* d_in, const void* d_surface, size_t width, size_t height, const acn_denoise_params* prm,
                        void* d_out_rgb, Call& c, bool from_stats )
{
    DenoiseSetup su;
    int st = denoise_check( h, d_in, d_surface, width, height, prm, d_out_rgb, c.opts, &su );
    if( st != ACN_OK ) return st;
    if( ( uintptr_t )d_surface % 16 ) return fail( ACN_ERR_ARG, "the surface records of a denoise call are read 16 bytes at a time: align the buffer" );
    if( from_stats && stats_buffer( d_in, width * height, "d_stats" ) != ACN_OK ) return ACN_ERR_ARG;
    if( ( st = call_begin( h, &c ) ) != ACN_OK ) return st;
    if( h->d_denoise.grow( width * height * ( size_t )ACN_DENOISE_SCRATCH_PER_PIXEL ) ) return ACN_ERR_DEVICE;
    if( from_stats )
        acn_launch_denoise_stats( ( const double* )d_in, ( const double* )d_surface, width, height, su.iterations, su.normal_power_log2, su.no_demodulate,
                                  su.sigma_plane, su.sigma_lum, h->dev.prm.background_color, h->d_denoise.get(), ( double* )d_out_rgb, c.stream );
    else
        acn_launch_denoise( ( const double* )d_in, ( const double* )d_surface, width, height, su.iterations, su.normal_power_log2, su.no_demodulate,
                            su.sigma_plane, su.sigma_lum, h->d_denoise.get(), ( double* )d_out_rgb, c.stream );
    HIP_TRY( hipGetLastError() );
    return call_end( c );
}

/* the two host forms.  The plain filter works in place on the copy of the frame; the statistics need a frame beside them */
static int denoise_host( acn_scene_handle* h, const double* in, const double* surface, size_t width, size_t height, const acn_denoise_params* prm,
                         double* out_rgb, const acn_render_opts* opts, bool from_stats )
{
    Call c( opts );
    DenoiseSetup su;
    int st = denoise_check( h, in, surface, width, height, prm, out_rgb, c.opts, &su );
    if( st != ACN_OK ) return st;
    const size_t n = width * height, rgb_bytes = sizeof( double ) * 3 * n;
    HostCall hc( h );
    void* d_in = from_stats ? hc.in( in, sizeof( double ) * ACN_STATS_STRIDE * n ) : hc.inout( in, out_rgb, rgb_bytes );
    void* d_surf = hc.in( surface, sizeof( double ) * ACN_SURF_STRIDE * n );
    void* d_rgb = from_stats ? hc.out( out_rgb, rgb_bytes ) : d_in;
    c.opts.stream = nullptr;
    return hc.run( [ & ] { return denoise_dev( h, d_in, d_surf, width, height, prm, d_rgb, c, from_stats ); } );
}

extern "C" int acn_denoise_dev( acn_scene_handle* h, const void* d_linear_rgb, const void* d_surface, size_t width, size_t height,
                                const acn_denoise_params* prm, void* d_out_rgb, const acn_render_opts* opts )
{
    Call c( opts );
    return denoise_dev( h, d_linear_rgb, d_surface, width, height, prm, d_out_rgb, c, false );
}

extern "C" int acn_denoise( acn_scene_handle* h, const double* linear_rgb, const double* surface, size_t width, size_t height,
                            const acn_denoise_params* prm, double* out_rgb, const acn_render_opts* opts )
{
    return denoise_host( h, linear_rgb, surface, width, height, prm, out_rgb, opts, false );
}

extern "C" int acn_denoise_stats_dev( acn_scene_handle* h, const void* d_stats, const void* d_surface, size_t width, size_t height,
                                      const acn_denoise_params* prm, void* d_out_rgb, const acn_render_opts* opts )
{
    Call c( opts );
    return denoise_dev( h, d_stats, d_surface, width, height, prm, d_out_rgb, c, true );
}

extern "C" int acn_denoise_stats( acn_scene_handle* h, const double* stats, const double* surface, size_t width, size_t height,
                                  const acn_denoise_params* prm, double* out_rgb, const acn_render_opts* opts )
{
    return denoise_host( h, stats, surface, width, height, prm, out_rgb, opts, true );
}

/* ---- filling a sparse frame (k_fill.hip; every check: acn_fill_host.h) ---- */
static int fill_check( const acn_scene_handle* h, const void* stats, const void* surface, size_t width, size_t height, const acn_fill_params* prm,
                       const void* out_stats, const void* out_need, const acn_render_opts& opts, FillSetup* su )
{
    std::string msg;
    return acn_fill_check( h != nullptr, stats, surface, width, height, prm, out_stats, out_need, opts.shard_world, su, &msg ) == ACN_OK
           ? ACN_OK : fail( ACN_ERR_ARG, msg );
}

static int fill_dev( acn_scene_handle* h, const void* d_stats, const void* d_surface, size_t width, size_t height, const acn_fill_params* prm,
                     void* d_out_stats, void* d_out_need, Call& c )
{
    FillSetup su;
    int st = fill_check( h, d_stats, d_surface, width, height, prm, d_out_stats, d_out_need, c.opts, &su );
    if( st != ACN_OK ) return st;
    if( ( st = call_begin( h, &c ) ) != ACN_OK ) return st;
    if( h->d_denoise.grow( width * height * ( size_t )ACN_DENOISE_SCRATCH_PER_PIXEL ) ) return ACN_ERR_DEVICE;
    acn_launch_fill_stats( ( const double* )d_stats, ( const double* )d_surface, width, height, su.radius, su.normal_power_log2, su.no_demodulate,
                           su.sigma_px, su.sigma_plane, h->dev.prm.background_color, h->d_denoise.get(), ( double* )d_out_stats, ( double* )d_out_need, c.stream );
    HIP_TRY( hipGetLastError() );
    return call_end( c );
}

extern "C" int acn_fill_stats_dev( acn_scene_handle* h, const void* d_stats, const void* d_surface, size_t width, size_t height,
                                   const acn_fill_params* prm, void* d_out_stats, void* d_out_need, const acn_render_opts* opts )
{
    Call c( opts );
    return fill_dev( h, d_stats, d_surface, width, height, prm, d_out_stats, d_out_need, c );
}

extern "C" int acn_fill_stats( acn_scene_handle* h, const double* stats, const double* surface, size_t width, size_t height,
                               const acn_fill_params* prm, double* out_stats, double* out_need, const acn_render_opts* opts )
{
    Call c( opts );
    FillSetup su;
    int st = fill_check( h, stats, surface, width, height, prm, out_stats, out_need, c.opts, &su );
    if( st != ACN_OK ) return st;
    const size_t n = width * height;
    HostCall hc( h );
    void* d_stats = hc.in( stats, sizeof( double ) * ACN_STATS_STRIDE * n );
    void* d_surf = hc.in( surface, sizeof( double ) * ACN_SURF_STRIDE * n );
    void* d_out = hc.out( out_stats, sizeof( double ) * ACN_STATS_STRIDE * n );
    void* d_need = hc.out( out_need, sizeof( double ) * n );
    c.opts.stream = nullptr;
    return hc.run( [ & ] { return fill_dev( h, d_stats, d_surf, width, height, prm, d_out, d_need, c ); } );
}

/* ---- the thin-lens camera (k_lens.hip) ---- */

/* every check of a lens call's parameters: on the host, before the handle is touched.  window: the samples an acn_lens_rays call asks for */
static int lens_check( const acn_scene_handle* h, const acn_lens_params* prm, const uint32_t* window, LensSetup* ls )
{
    if( !h ) return fail( ACN_ERR_ARG, "null argument" );
    acn_lens_params p;
    std::string msg;
    if( acn_lens_params_read( prm, &p, &msg ) != ACN_OK ) return fail( ACN_ERR_ARG, msg );   /* (acn_stats_host.h: the members alone) */
    if( p.aperture_radius > 0 && !( h->dev.prm.camera_focal_length > 0 ) ) return fail( ACN_ERR_ARG, "an open aperture needs a camera_focal_length above 0: the plane in focus lies in front of the camera" );
    ls->samples = p.samples ? p.samples : ACN_LENS_DEFAULT_SAMPLES;
    ls->jitter = ( p.flags & ACN_LENS_JITTER ) ? 1u : 0u;
    ls->seed = ACN_LENS_SEED + ( uint64_t )p.seed;
    ls->aperture_radius = p.aperture_radius;
    ls->focus_distance = p.aperture_radius > 0 ? p.focus_distance : 0.0;
    if( window )
    {
        if( window[ 1 ] == 0 ) return fail( ACN_ERR_ARG, "n_samples is 0" );
        if( ( uint64_t )window[ 0 ] + window[ 1 ] > ls->samples ) return fail( ACN_ERR_ARG, "first_sample + n_samples is above the " + std::to_string( ls->samples ) + " samples of the lens" );
    }
    return ACN_OK;
}

/* the checks an acn_lens_rays call makes before its n == 0 return, in either form */
static int lens_rays_check( const acn_scene_handle* h, const void* pos_xy, size_t n, const acn_lens_params* prm, uint32_t first_sample,
                            uint32_t n_samples, const void* out_rays, LensSetup* ls )
{
    if( !h || ( n && ( !pos_xy || !out_rays ) ) ) return fail( ACN_ERR_ARG, "null argument" );
    const uint32_t window[ 2 ] = { first_sample, n_samples };
    int st = lens_check( h, prm, window, ls );
    if( st != ACN_OK ) return st;
    if( n > 0xFFFFFF00ull / n_samples ) return fail( ACN_ERR_ARG, "too many rays in one call" );
    return ACN_OK;
}

extern "C" int acn_lens_rays_dev( acn_scene_handle* h, const void* d_pos_xy, size_t n, const acn_lens_params* prm, uint32_t first_sample,
                                  uint32_t n_samples, void* d_out_rays, const acn_render_opts* opts )
{
    Call c( opts );
    LensSetup ls;
    int st = lens_rays_check( h, d_pos_xy, n, prm, first_sample, n_samples, d_out_rays, &ls );
    if( st != ACN_OK || n == 0 ) return st;
    if( ( st = call_begin( h, &c ) ) != ACN_OK ) return st;
    acn_launch_lens_rays( h->dev, ( const double* )d_pos_xy, 0, n, ls, first_sample, n_samples, ( double* )d_out_rays, c.stream );
    HIP_TRY( hipGetLastError() );
    return call_end( c );
}

extern "C" int acn_lens_rays( acn_scene_handle* h, const double* pos_xy, size_t n, const acn_lens_params* prm, uint32_t first_sample,
                              uint32_t n_samples, double* out_rays )
{
    LensSetup ls;
    int st = lens_rays_check( h, pos_xy, n, prm, first_sample, n_samples, out_rays, &ls );
    if( st != ACN_OK || n == 0 ) return st;
    return host_in_out( h, pos_xy, sizeof( double ) * 2 * n, out_rays, sizeof( double ) * 6 * n_samples * n, [ & ]( void* d_pos, void* d_out )
    {
        return acn_lens_rays_dev( h, d_pos, n, prm, first_sample, n_samples, d_out, nullptr );
    } );
}

/* The slice loop of every lens call, after the call's checks and with n > 0: d_pos_xy, or null for the pixel centres from `first` on.
 * A slice is acn_lenssurf_slice positions; its rays go into the handle's slice buffers once, and from them come the per-ray products
 * the call wants: the radiance, by the ray path of acn_render_rays_dev (linear; its validity kernel left out: the rays are valid by
 * construction), the surface records, by the surface kernel of acn_surface_rays (likewise), or both.  reduce( base, cnt, d_rad, d_surf )
 * launches the call's reduction(s) of positions [ base, base + cnt ) on c.stream; a product not wanted is null.  Cancel is polled iff
 * the slice renders: a call for records alone reads only `stream` of its options. */
struct LensProducts { bool radiance, surface; uint32_t mode; };   /* mode: of the surface records */

template< class Reduce >
static int lens_slices( acn_scene_handle* h, const double* d_pos_xy, size_t first, size_t n, const LensSetup& ls, Call& c, LensProducts want, Reduce reduce )
{
    int st = call_begin( h, &c );
    if( st != ACN_OK ) return st;
    const uint32_t K = ls.samples;
    const size_t slice = acn_lenssurf_slice( h->tun.lens_slice_rays, K, n );
    if( h->d_lens_rays.grow( sizeof( double ) * 6 * slice * K ) || ( want.radiance && h->d_lens_rad.grow( sizeof( double ) * 3 * slice * K ) ) ||
        ( want.surface && h->d_lens_surf.grow( sizeof( double ) * ACN_SURF_STRIDE * slice * K ) ) ) return ACN_ERR_DEVICE;
    double* const d_rays = h->d_lens_rays.get();
    double* const d_rad = want.radiance ? h->d_lens_rad.get() : nullptr;
    double* const d_surf = want.surface ? h->d_lens_surf.get() : nullptr;
    SceneArgs s;
    if( want.surface && ( st = surface_flags_begin( h, &s ) ) != ACN_OK ) return st;
    acn_render_opts ray_opts = c.opts;
    ray_opts.flags |= ACN_OPT_LINEAR_OUT;
    for( size_t base = 0; base < n; base += slice )
    {
        if( want.radiance && c.opts.cancel && *c.opts.cancel ) return fail( ACN_ERR_CANCELLED, "cancelled" );
        const size_t cnt = n - base < slice ? n - base : slice;
        acn_launch_lens_rays( h->dev, d_pos_xy ? d_pos_xy + 2 * base : nullptr, first + base, cnt, ls, 0, K, d_rays, c.stream );
        HIP_TRY( hipGetLastError() );
        if( want.radiance && ( st = render_dispatch( h, primary_rays( d_rays ), cnt * K, d_rad, &ray_opts, c.stream ) ) != ACN_OK ) return st;
        if( want.surface )
        {
            acn_launch_surface( want.mode, h->scene.lds_bytes != 0, machine_lds_bytes( h->scene ), c.stream, s, d_rays, nullptr, cnt * K, d_surf );
            HIP_TRY( hipGetLastError() );
        }
        reduce( base, cnt, d_rad, d_surf );
        HIP_TRY( hipGetLastError() );
    }
    return want.surface ? surface_flags_end( h, c ) : call_end( c );
}

static int lens_stats_by_samples() { return fail( ACN_ERR_ARG, "lens statistics are not sharded by samples (ACN_SHARD_SAMPLES): deviations of partial radiances mean nothing" ); }

/* a lens call after its null checks: the ordered mean of each position's radiances, with_stats their statistics records beside it */
static int render_lens( acn_scene_handle* h, const double* d_pos_xy, size_t first, size_t n, const acn_lens_params* prm, double* d_out_rgb,
                        Call& c, double* d_stats = nullptr, bool with_stats = false )
{
    LensSetup ls;
    int st = lens_check( h, prm, nullptr, &ls );
    if( st != ACN_OK ) return st;
    const acn_render_opts& o = c.opts;
    const int linear = ( o.flags & ACN_OPT_LINEAR_OUT ) ? 1 : 0;
    if( o.shard_mode > ACN_SHARD_SAMPLES ) return fail( ACN_ERR_ARG, "unknown shard_mode" );
    if( o.shard_mode == ACN_SHARD_SAMPLES && o.shard_world > 1 )
    {
        if( o.shard_rank >= o.shard_world ) return fail( ACN_ERR_ARG, "shard_rank >= shard_world" );
        if( with_stats ) return lens_stats_by_samples();
        if( !linear ) return fail( ACN_ERR_ARG, "a lens call sharded by samples gives partial means: it needs ACN_OPT_LINEAR_OUT" );
    }
    if( o.cancel && *o.cancel ) return fail( ACN_ERR_CANCELLED, "cancelled" );
    if( n == 0 ) return ACN_OK;
    return lens_slices( h, d_pos_xy, first, n, ls, c, { true, false, 0 }, [ & ]( size_t base, size_t cnt, const double* d_rad, const double* )
    {
        if( with_stats )
            acn_launch_lens_reduce_stats( d_rad, cnt, ls.samples, h->dev.prm.gamma, linear, d_out_rgb ? d_out_rgb + 3 * base : nullptr,
                                          d_stats + ( size_t )ACN_STATS_STRIDE * base, c.stream );
        else
            acn_launch_lens_reduce( d_rad, cnt, ls.samples, h->dev.prm.gamma, linear, d_out_rgb + 3 * base, c.stream );
    } );
}

extern "C" int acn_render_lens_dev( acn_scene_handle* h, const void* d_pos_xy, size_t n, const acn_lens_params* prm, void* d_out_rgb,
                                    const acn_render_opts* opts )
{
    Call c( opts );
    if( !h || ( n && ( !d_pos_xy || !d_out_rgb ) ) ) return fail( ACN_ERR_ARG, "null argument" );
    return render_lens( h, ( const double* )d_pos_xy, 0, n, prm, ( double* )d_out_rgb, c );
}

extern "C" int acn_render_lens_main_pass_dev( acn_scene_handle* h, size_t first, size_t count, const acn_lens_params* prm, void* d_out_rgb,
                                              const acn_render_opts* opts )
{
    Call c( opts );
    if( !h || ( count && !d_out_rgb ) ) return fail( ACN_ERR_ARG, "null argument" );
    int st = pixel_range_check( h, first, count );
    return st != ACN_OK ? st : render_lens( h, nullptr, first, count, prm, ( double* )d_out_rgb, c );
}

extern "C" int acn_render_lens( acn_scene_handle* h, const double* pos_xy, size_t n, const acn_lens_params* prm, double* out_rgb,
                                const acn_render_opts* opts )
{
    Call c( opts );
    if( !h || ( n && ( !pos_xy || !out_rgb ) ) ) return fail( ACN_ERR_ARG, "null argument" );
    LensSetup ls;
    int st = lens_check( h, prm, nullptr, &ls );   /* (before the buffers are made; the device call checks the rest before it writes) */
    if( st != ACN_OK || n == 0 ) return st;
    c.opts.stream = nullptr;
    return host_in_out( h, pos_xy, sizeof( double ) * 2 * n, out_rgb, sizeof( double ) * 3 * n,
                        [ & ]( void* d_pos, void* d_out ) { return acn_render_lens_dev( h, d_pos, n, prm, d_out, &c.opts ); } );
}

/* ---- lens sample statistics (k_lens.hip, k_denoise.hip) ---- */
extern "C" int acn_render_lens_stats_dev( acn_scene_handle* h, const void* d_pos_xy, size_t n, const acn_lens_params* prm, void* d_out_rgb,
                                          void* d_stats, const acn_render_opts* opts )
{
    Call c( opts );
    if( !h || ( n && ( !d_pos_xy || !d_stats ) ) ) return fail( ACN_ERR_ARG, "null argument" );
    if( stats_buffer( d_stats, n, "d_stats" ) != ACN_OK ) return ACN_ERR_ARG;
    return render_lens( h, ( const double* )d_pos_xy, 0, n, prm, ( double* )d_out_rgb, c, ( double* )d_stats, true );
}

extern "C" int acn_render_lens_stats_main_pass_dev( acn_scene_handle* h, size_t first, size_t count, const acn_lens_params* prm, void* d_out_rgb,
                                                    void* d_stats, const acn_render_opts* opts )
{
    Call c( opts );
    if( !h || ( count && !d_stats ) ) return fail( ACN_ERR_ARG, "null argument" );
    if( stats_buffer( d_stats, count, "d_stats" ) != ACN_OK ) return ACN_ERR_ARG;
    int st = pixel_range_check( h, first, count );
    return st != ACN_OK ? st : render_lens( h, nullptr, first, count, prm, ( double* )d_out_rgb, c, ( double* )d_stats, true );
}

extern "C" int acn_render_lens_stats( acn_scene_handle* h, const double* pos_xy, size_t n, const acn_lens_params* prm, double* out_rgb,
                                      double* stats, const acn_render_opts* opts )
{
    Call c( opts );
    if( !h || ( n && ( !pos_xy || !stats ) ) ) return fail( ACN_ERR_ARG, "null argument" );
    LensSetup ls;
    int st = lens_check( h, prm, nullptr, &ls );   /* (before the buffers are made; the device call checks the rest before it writes) */
    if( st != ACN_OK ) return st;
    if( c.opts.shard_mode == ACN_SHARD_SAMPLES && c.opts.shard_world > 1 ) return lens_stats_by_samples();
    if( n == 0 ) return ACN_OK;
    HostCall hc( h );
    void* d_pos = hc.in( pos_xy, sizeof( double ) * 2 * n );
    void* d_out = hc.out( out_rgb, sizeof( double ) * 3 * n );
    void* d_st = hc.out( stats, sizeof( double ) * ACN_STATS_STRIDE * n );
    c.opts.stream = nullptr;
    return hc.run( [ & ] { return acn_render_lens_stats_dev( h, d_pos, n, prm, d_out, d_st, &c.opts ); } );
}

extern "C" int acn_lens_stats_merge_dev( acn_scene_handle* h, void* d_acc, size_t n_acc, const void* d_part, size_t n_part,
                                         const int64_t* d_index, const acn_render_opts* opts )
{
    Call c( opts );
    if( !h ) return fail( ACN_ERR_ARG, "null argument" );
    if( c.opts.shard_world > 1 ) return fail( ACN_ERR_ARG, "a merge of lens statistics is not sharded" );
    if( stats_buffer( d_acc, n_acc, "d_acc" ) != ACN_OK || stats_buffer( d_part, n_part, "d_part" ) != ACN_OK ) return ACN_ERR_ARG;
    if( !d_index && n_part > n_acc ) return fail( ACN_ERR_ARG, "a merge without an index needs n_part <= n_acc" );
    if( ( uintptr_t )d_index % 8 ) return fail( ACN_ERR_ARG, "d_index is an array of int64_t: align the buffer" );
    if( n_part == 0 || n_acc == 0 ) return ACN_OK;
    int st = call_begin( h, &c );
    if( st != ACN_OK ) return st;
    acn_launch_stats_merge( ( double* )d_acc, n_acc, ( const double* )d_part, n_part, d_index, c.stream );
    HIP_TRY( hipGetLastError() );
    return call_end( c );
}

extern "C" int acn_lens_stats_merge( acn_scene_handle* h, double* acc, size_t n_acc, const double* part, size_t n_part,
                                     const int64_t* index, const acn_render_opts* opts )
{
    Call c( opts );
    if( !h || ( n_acc && !acc ) || ( n_part && !part ) ) return fail( ACN_ERR_ARG, "null argument" );
    if( c.opts.shard_world > 1 ) return fail( ACN_ERR_ARG, "a merge of lens statistics is not sharded" );
    std::string msg;
    if( acn_stats_index_check( index, n_part, n_acc, &msg ) != ACN_OK ) return fail( ACN_ERR_ARG, msg );
    if( n_part == 0 || n_acc == 0 ) return ACN_OK;
    const size_t rec = sizeof( double ) * ACN_STATS_STRIDE;
    HostCall hc( h );
    void* d_acc = hc.inout( acc, acc, rec * n_acc );
    void* d_part = hc.in( part, rec * n_part );
    void* d_index = index ? hc.in( index, sizeof( int64_t ) * n_part ) : nullptr;
    c.opts.stream = nullptr;
    return hc.run( [ & ] { return acn_lens_stats_merge_dev( h, d_acc, n_acc, d_part, n_part, ( const int64_t* )d_index, &c.opts ); } );
}

extern "C" int acn_lens_stats_resolve_dev( acn_scene_handle* h, const void* d_stats, size_t n, void* d_out_rgb, void* d_out_noise,
                                           const acn_render_opts* opts )
{
    Call c( opts );
    if( !h || ( n && !d_stats ) ) return fail( ACN_ERR_ARG, "null argument" );
    if( c.opts.shard_world > 1 ) return fail( ACN_ERR_ARG, "a resolve of lens statistics is not sharded" );
    if( stats_buffer( d_stats, n, "d_stats" ) != ACN_OK ) return ACN_ERR_ARG;
    if( n == 0 || ( !d_out_rgb && !d_out_noise ) ) return ACN_OK;
    int st = call_begin( h, &c );
    if( st != ACN_OK ) return st;
    acn_launch_stats_resolve( ( const double* )d_stats, n, h->dev.prm.background_color, h->dev.prm.gamma, ( c.opts.flags & ACN_OPT_LINEAR_OUT ) ? 1 : 0,
                              ( double* )d_out_rgb, ( double* )d_out_noise, c.stream );
    HIP_TRY( hipGetLastError() );
    return call_end( c );
}

/* ---- lens surface records (k_lens_surface.hip; the checks that need no handle: acn_lenssurf_host.h) ---- */
extern "C" int acn_surface_reduce_dev( acn_scene_handle* h, const void* d_records, size_t n, uint32_t K, void* d_out, const acn_render_opts* opts )
{
    Call c( opts );
    std::string msg;
    if( acn_lenssurf_reduce_check( h != nullptr, d_records, n, K, d_out, c.opts.shard_world, &msg ) != ACN_OK ) return fail( ACN_ERR_ARG, msg );
    if( n == 0 ) return ACN_OK;
    int st = call_begin( h, &c );
    if( st != ACN_OK ) return st;
    acn_launch_surface_reduce( ( const double* )d_records, n, K, ( double* )d_out, c.stream );
    HIP_TRY( hipGetLastError() );
    return call_end( c );
}

extern "C" int acn_surface_reduce( acn_scene_handle* h, const double* records, size_t n, uint32_t K, double* out, const acn_render_opts* opts )
{
    Call c( opts );
    std::string msg;
    if( acn_lenssurf_reduce_check( h != nullptr, records, n, K, out, c.opts.shard_world, &msg ) != ACN_OK ) return fail( ACN_ERR_ARG, msg );
    if( n == 0 ) return ACN_OK;
    const size_t rec = sizeof( double ) * ACN_SURF_STRIDE;
    return host_in_out( h, records, rec * K * n, out, rec * n,
                        [ & ]( void* d_in, void* d_out ) { return acn_surface_reduce_dev( h, d_in, n, K, d_out, nullptr ); } );
}

/* a lens surface call after its checks: the aggregate record of each position's records */
static int surface_lens( acn_scene_handle* h, const double* d_pos_xy, size_t first, size_t n, const acn_lens_params* prm, uint32_t mode, double* d_out, Call& c )
{
    LensSetup ls;
    int st = lens_check( h, prm, nullptr, &ls );   /* (the members again, and the one check that needs the scene: the focal length) */
    if( st != ACN_OK || n == 0 ) return st;
    return lens_slices( h, d_pos_xy, first, n, ls, c, { false, true, mode }, [ & ]( size_t base, size_t cnt, const double*, const double* d_surf )
    {
        acn_launch_surface_reduce( d_surf, cnt, ls.samples, d_out + ( size_t )ACN_SURF_STRIDE * base, c.stream );
    } );
}

extern "C" int acn_surface_lens_dev( acn_scene_handle* h, const void* d_pos_xy, size_t n, const acn_lens_params* prm, uint32_t mode, void* d_out,
                                     const acn_render_opts* opts )
{
    Call c( opts );
    std::string msg;
    acn_lens_params p;
    if( acn_lenssurf_lens_check( h != nullptr, true, d_pos_xy, n, prm, mode, d_out, c.opts.shard_world, &p, &msg ) != ACN_OK ) return fail( ACN_ERR_ARG, msg );
    return surface_lens( h, ( const double* )d_pos_xy, 0, n, prm, mode, ( double* )d_out, c );
}

extern "C" int acn_surface_lens_main_pass_dev( acn_scene_handle* h, size_t first, size_t count, const acn_lens_params* prm, uint32_t mode, void* d_out,
                                               const acn_render_opts* opts )
{
    Call c( opts );
    std::string msg;
    acn_lens_params p;
    if( acn_lenssurf_lens_check( h != nullptr, false, nullptr, count, prm, mode, d_out, c.opts.shard_world, &p, &msg ) != ACN_OK ) return fail( ACN_ERR_ARG, msg );
    int st = pixel_range_check( h, first, count );
    return st != ACN_OK ? st : surface_lens( h, nullptr, first, count, prm, mode, ( double* )d_out, c );
}

extern "C" int acn_surface_lens( acn_scene_handle* h, const double* pos_xy, size_t n, const acn_lens_params* prm, uint32_t mode, double* out,
                                 const acn_render_opts* opts )
{
    Call c( opts );
    std::string msg;
    acn_lens_params p;
    if( acn_lenssurf_lens_check( h != nullptr, true, pos_xy, n, prm, mode, out, c.opts.shard_world, &p, &msg ) != ACN_OK ) return fail( ACN_ERR_ARG, msg );
    LensSetup ls;
    int st = lens_check( h, prm, nullptr, &ls );   /* (before the buffers are made) */
    if( st != ACN_OK || n == 0 ) return st;
    return host_in_out( h, pos_xy, sizeof( double ) * 2 * n, out, sizeof( double ) * ACN_SURF_STRIDE * n,
                        [ & ]( void* d_pos, void* d_out ) { return acn_surface_lens_dev( h, d_pos, n, prm, mode, d_out, nullptr ); } );
}

/* ---- layered lens records and their filter (k_lens_layers.hip, k_denoise_layers.hip; the checks that need no handle: acn_layers_host.h) ---- */
extern "C" int acn_lens_layers_reduce_dev( acn_scene_handle* h, const void* d_records, const void* d_radiance, size_t n, uint32_t K, void* d_out_surface,
                                           void* d_out_stats, const acn_render_opts* opts )
{
    Call c( opts );
    std::string msg;
    if( acn_layers_reduce_check( h != nullptr, d_records, d_radiance, n, K, d_out_surface, d_out_stats, c.opts.shard_world, &msg ) != ACN_OK ) return fail( ACN_ERR_ARG, msg );
    if( n == 0 ) return ACN_OK;
    int st = call_begin( h, &c );
    if( st != ACN_OK ) return st;
    acn_launch_lens_layers( ( const double* )d_records, ( const double* )d_radiance, n, K, ( double* )d_out_surface, n, ( double* )d_out_stats, n, c.stream );
    HIP_TRY( hipGetLastError() );
    return call_end( c );
}

extern "C" int acn_lens_layers_reduce( acn_scene_handle* h, const double* records, const double* radiance, size_t n, uint32_t K, double* out_surface,
                                       double* out_stats, const acn_render_opts* opts )
{
    Call c( opts );
    std::string msg;
    if( acn_layers_reduce_check( h != nullptr, records, radiance, n, K, out_surface, out_stats, c.opts.shard_world, &msg ) != ACN_OK ) return fail( ACN_ERR_ARG, msg );
    if( n == 0 ) return ACN_OK;
    HostCall hc( h );
    void* d_rec = hc.in( records, sizeof( double ) * ACN_SURF_STRIDE * K * n );
    void* d_rad = hc.in( radiance, sizeof( double ) * 3 * K * n );
    void* d_surf = hc.out( out_surface, sizeof( double ) * ACN_SURF_STRIDE * 2 * n );
    void* d_st = hc.out( out_stats, sizeof( double ) * ACN_STATS_STRIDE * 3 * n );
    return hc.run( [ & ] { return acn_lens_layers_reduce_dev( h, d_rec, d_rad, n, K, d_surf, d_st, nullptr ); } );
}

/* a layered lens call after its checks: the ordered mean of render_lens (if d_out_rgb) and the split of each position's records and
 * radiances into the caller's planes [ . ][ n ] */
static int render_lens_layers( acn_scene_handle* h, const double* d_pos_xy, size_t first, size_t n, const acn_lens_params* prm, uint32_t mode,
                               double* d_out_rgb, double* d_out_surface, double* d_out_stats, Call& c )
{
    LensSetup ls;
    int st = lens_check( h, prm, nullptr, &ls );   /* (the members again, and the one check that needs the scene: the focal length) */
    if( st != ACN_OK ) return st;
    const acn_render_opts& o = c.opts;
    const int linear = ( o.flags & ACN_OPT_LINEAR_OUT ) ? 1 : 0;
    if( o.cancel && *o.cancel ) return fail( ACN_ERR_CANCELLED, "cancelled" );
    if( n == 0 ) return ACN_OK;
    return lens_slices( h, d_pos_xy, first, n, ls, c, { true, true, mode }, [ & ]( size_t base, size_t cnt, const double* d_rad, const double* d_surf )
    {
        if( d_out_rgb ) acn_launch_lens_reduce( d_rad, cnt, ls.samples, h->dev.prm.gamma, linear, d_out_rgb + 3 * base, c.stream );
        acn_launch_lens_layers( d_surf, d_rad, cnt, ls.samples, d_out_surface + ( size_t )ACN_SURF_STRIDE * base, n,
                                d_out_stats + ( size_t )ACN_STATS_STRIDE * base, n, c.stream );
    } );
}

extern "C" int acn_render_lens_layers_dev( acn_scene_handle* h, const void* d_pos_xy, size_t n, const acn_lens_params* prm, uint32_t mode,
                                           void* d_out_rgb, void* d_out_surface, void* d_out_stats, const acn_render_opts* opts )
{
    Call c( opts );
    std::string msg;
    acn_lens_params p;
    if( acn_layers_lens_check( h != nullptr, true, d_pos_xy, n, prm, mode, d_out_surface, d_out_stats, c.opts.shard_mode, c.opts.shard_rank,
                               c.opts.shard_world, &p, &msg ) != ACN_OK ) return fail( ACN_ERR_ARG, msg );
    return render_lens_layers( h, ( const double* )d_pos_xy, 0, n, prm, mode, ( double* )d_out_rgb, ( double* )d_out_surface, ( double* )d_out_stats, c );
}

extern "C" int acn_render_lens_layers_main_pass_dev( acn_scene_handle* h, size_t first, size_t count, const acn_lens_params* prm, uint32_t mode,
                                                     void* d_out_rgb, void* d_out_surface, void* d_out_stats, const acn_render_opts* opts )
{
    Call c( opts );
    std::string msg;
    acn_lens_params p;
    if( acn_layers_lens_check( h != nullptr, false, nullptr, count, prm, mode, d_out_surface, d_out_stats, c.opts.shard_mode, c.opts.shard_rank,
                               c.opts.shard_world, &p, &msg ) != ACN_OK ) return fail( ACN_ERR_ARG, msg );
    int st = pixel_range_check( h, first, count );
    return st != ACN_OK ? st : render_lens_layers( h, nullptr, first, count, prm, mode, ( double* )d_out_rgb, ( double* )d_out_surface, ( double* )d_out_stats, c );
}

extern "C" int acn_render_lens_layers( acn_scene_handle* h, const double* pos_xy, size_t n, const acn_lens_params* prm, uint32_t mode, double* out_rgb,
                                       double* out_surface, double* out_stats, const acn_render_opts* opts )
{
    Call c( opts );
    std::string msg;
    acn_lens_params p;
    if( acn_layers_lens_check( h != nullptr, true, pos_xy, n, prm, mode, out_surface, out_stats, c.opts.shard_mode, c.opts.shard_rank, c.opts.shard_world,
                               &p, &msg ) != ACN_OK ) return fail( ACN_ERR_ARG, msg );
    LensSetup ls;
    int st = lens_check( h, prm, nullptr, &ls );   /* (before the buffers are made) */
    if( st != ACN_OK || n == 0 ) return st;
    HostCall hc( h );
    void* d_pos = hc.in( pos_xy, sizeof( double ) * 2 * n );
    void* d_rgb = hc.out( out_rgb, sizeof( double ) * 3 * n );
    void* d_surf = hc.out( out_surface, sizeof( double ) * ACN_SURF_STRIDE * 2 * n );
    void* d_st = hc.out( out_stats, sizeof( double ) * ACN_STATS_STRIDE * 3 * n );
    c.opts.stream = nullptr;
    return hc.run( [ & ] { return acn_render_lens_layers_dev( h, d_pos, n, prm, mode, d_rgb, d_surf, d_st, &c.opts ); } );
}

extern "C" int acn_denoise_layers_dev( acn_scene_handle* h, const void* d_stats, const void* d_surface, size_t width, size_t height,
                                       const acn_denoise_params* prm, void* d_out_rgb, const acn_render_opts* opts )
{
    Call c( opts );
    DenoiseSetup su;
    int st = denoise_check( h, d_stats, d_surface, width, height, prm, d_out_rgb, c.opts, &su );
    if( st != ACN_OK ) return st;
    std::string msg;
    if( acn_layers_denoise_check( d_stats, d_surface, &msg ) != ACN_OK ) return fail( ACN_ERR_ARG, msg );
    if( ( st = call_begin( h, &c ) ) != ACN_OK ) return st;
    if( h->d_denoise.grow( width * height * ( size_t )ACN_DENOISE_LAYERS_SCRATCH_PER_PIXEL ) ) return ACN_ERR_DEVICE;
    acn_launch_denoise_layers( ( const double* )d_stats, ( const double* )d_surface, width, height, su.iterations, su.normal_power_log2, su.no_demodulate,
                               su.sigma_plane, su.sigma_lum, h->dev.prm.background_color, h->d_denoise.get(), ( double* )d_out_rgb, c.stream );
    HIP_TRY( hipGetLastError() );
    return call_end( c );
}

extern "C" int acn_denoise_layers( acn_scene_handle* h, const double* stats, const double* surface, size_t width, size_t height,
                                   const acn_denoise_params* prm, double* out_rgb, const acn_render_opts* opts )
{
    Call c( opts );
    DenoiseSetup su;
    int st = denoise_check( h, stats, surface, width, height, prm, out_rgb, c.opts, &su );
    if( st != ACN_OK ) return st;
    const size_t n = width * height;
    HostCall hc( h );
    void* d_st = hc.in( stats, sizeof( double ) * ACN_STATS_STRIDE * 3 * n );
    void* d_surf = hc.in( surface, sizeof( double ) * ACN_SURF_STRIDE * 2 * n );
    void* d_rgb = hc.out( out_rgb, sizeof( double ) * 3 * n );
    c.opts.stream = nullptr;
    return hc.run( [ & ] { return acn_denoise_layers_dev( h, d_st, d_surf, width, height, prm, d_rgb, &c.opts ); } );
}

/* ---- layered records merged across passes and resolved (k_lens_layers_merge.hip; the checks: acn_layers_host.h) ---- */
extern "C" int acn_lens_layers_merge_dev( acn_scene_handle* h, void* d_acc_surface, void* d_acc_stats, size_t n_acc, const void* d_part_surface,
                                          const void* d_part_stats, size_t n_part, const int64_t* d_index, const acn_render_opts* opts )
{
    Call c( opts );
    std::string msg;
    if( acn_layers_merge_check( h != nullptr, d_acc_surface, d_acc_stats, n_acc, d_part_surface, d_part_stats, n_part, d_index, false,
                                c.opts.shard_world, &msg ) != ACN_OK ) return fail( ACN_ERR_ARG, msg );
    if( n_part == 0 || n_acc == 0 ) return ACN_OK;
    int st = call_begin( h, &c );
    if( st != ACN_OK ) return st;
    acn_launch_lens_layers_merge( ( double* )d_acc_surface, ( double* )d_acc_stats, n_acc, ( const double* )d_part_surface, ( const double* )d_part_stats,
                                  n_part, d_index, c.stream );
    HIP_TRY( hipGetLastError() );
    return call_end( c );
}

extern "C" int acn_lens_layers_merge( acn_scene_handle* h, double* acc_surface, double* acc_stats, size_t n_acc, const double* part_surface,
                                      const double* part_stats, size_t n_part, const int64_t* index, const acn_render_opts* opts )
{
    Call c( opts );
    std::string msg;
    if( acn_layers_merge_check( h != nullptr, acc_surface, acc_stats, n_acc, part_surface, part_stats, n_part, index, true, c.opts.shard_world,
                                &msg ) != ACN_OK ) return fail( ACN_ERR_ARG, msg );
    if( n_part == 0 || n_acc == 0 ) return ACN_OK;
    const size_t srec = sizeof( double ) * ACN_SURF_STRIDE * ACN_LAYERS_SURFACE_PLANES, trec = sizeof( double ) * ACN_STATS_STRIDE * ACN_LAYERS_STATS_PLANES;
    HostCall hc( h );
    void* d_as = hc.inout( acc_surface, acc_surface, srec * n_acc );
    void* d_at = hc.inout( acc_stats, acc_stats, trec * n_acc );
    void* d_ps = hc.in( part_surface, srec * n_part );
    void* d_pt = hc.in( part_stats, trec * n_part );
    void* d_index = index ? hc.in( index, sizeof( int64_t ) * n_part ) : nullptr;
    c.opts.stream = nullptr;
    return hc.run( [ & ] { return acn_lens_layers_merge_dev( h, d_as, d_at, n_acc, d_ps, d_pt, n_part, ( const int64_t* )d_index, &c.opts ); } );
}

extern "C" int acn_lens_layers_resolve_dev( acn_scene_handle* h, const void* d_stats, size_t n, void* d_out_rgb, void* d_out_noise, void* d_out_pooled,
                                            const acn_render_opts* opts )
{
    Call c( opts );
    std::string msg;
    if( acn_layers_resolve_check( h != nullptr, d_stats, n, d_out_rgb, d_out_noise, d_out_pooled, c.opts.shard_world, &msg ) != ACN_OK ) return fail( ACN_ERR_ARG, msg );
    if( n == 0 || ( !d_out_rgb && !d_out_noise && !d_out_pooled ) ) return ACN_OK;
    int st = call_begin( h, &c );
    if( st != ACN_OK ) return st;
    acn_launch_lens_layers_resolve( ( const double* )d_stats, n, h->dev.prm.background_color, h->dev.prm.gamma, ( c.opts.flags & ACN_OPT_LINEAR_OUT ) ? 1 : 0,
                                    ( double* )d_out_rgb, ( double* )d_out_noise, ( double* )d_out_pooled, c.stream );
    HIP_TRY( hipGetLastError() );
    return call_end( c );
}

/* ---- projected points and reprojected statistics (k_reproject.hip; the checks that need no handle: acn_reproject_host.h) ---- */
extern "C" int acn_project_points_dev( acn_scene_handle* h, const void* d_points, size_t n, void* d_out_pos_xy, void* d_out_depth, const acn_render_opts* opts )
{
    Call c( opts );
    if( !h || ( n && ( !d_points || !d_out_pos_xy ) ) ) return fail( ACN_ERR_ARG, "null argument" );
    if( n == 0 ) return ACN_OK;
    if( n > 0xFFFFFF00ull ) return fail( ACN_ERR_ARG, "too many points in one call" );
    int st = call_begin( h, &c );
    if( st != ACN_OK ) return st;
    acn_launch_project_points( h->dev, ( const double* )d_points, n, ( double* )d_out_pos_xy, ( double* )d_out_depth, c.stream );
    HIP_TRY( hipGetLastError() );
    return call_end( c );
}

extern "C" int acn_project_points( acn_scene_handle* h, const double* points, size_t n, double* out_pos_xy, double* out_depth )
{
    if( !h || ( n && ( !points || !out_pos_xy ) ) ) return fail( ACN_ERR_ARG, "null argument" );
    if( n == 0 ) return ACN_OK;
    if( n > 0xFFFFFF00ull ) return fail( ACN_ERR_ARG, "too many points in one call" );
    HostCall hc( h );
    void* d_points = hc.in( points, sizeof( double ) * 3 * n );
    void* d_pos = hc.out( out_pos_xy, sizeof( double ) * 2 * n );
    void* d_depth = hc.out( out_depth, sizeof( double ) * n );
    return hc.run( [ & ] { return acn_project_points_dev( h, d_points, n, d_pos, d_depth, nullptr ); } );
}

/* every check of a reproject call, on the host before the handle is touched: those that need no handle, then what acn_scene_set_params
 * refuses of the previous frame's parameters */
static int reproject_check( const acn_scene_handle* h, const void* cur_surface, size_t n, const acn_params* prev_params, const void* prev_surface,
                            const void* prev_stats, const acn_reproject_params* prm, const void* out_stats, const void* out_motion,
                            const acn_render_opts& opts, ReprojectSetup* su )
{
    std::string msg;
    acn_reproject_params p;
    if( acn_reproject_check( h != nullptr, cur_surface, n, prev_params, prev_surface, prev_stats, prm, out_stats, out_motion, opts.shard_world,
                             &p, &msg ) != ACN_OK ) return fail( ACN_ERR_ARG, msg );
    if( acn_tables_validate_params( prev_params, &msg ) != ACN_OK ) return fail( ACN_ERR_ARG, "prev_params: " + msg );
    su->reject_kinds = p.reject_kinds; su->max_hops = p.max_hops;
    su->normal_min = p.normal_min; su->plane_tolerance = p.plane_tolerance; su->max_history = p.max_history;
    return ACN_OK;
}

extern "C" int acn_reproject_dev( acn_scene_handle* h, const void* d_cur_surface, size_t n, const acn_params* prev_params, const void* d_prev_surface,
                                  const void* d_prev_stats, const acn_reproject_params* prm, void* d_out_stats, void* d_out_motion,
                                  const acn_render_opts* opts )
{
    Call c( opts );
    ReprojectSetup su;
    int st = reproject_check( h, d_cur_surface, n, prev_params, d_prev_surface, d_prev_stats, prm, d_out_stats, d_out_motion, c.opts, &su );
    if( st != ACN_OK || n == 0 ) return st;
    if( ( st = call_begin( h, &c ) ) != ACN_OK ) return st;
    acn_launch_reproject( ( const double* )d_cur_surface, n, *prev_params, ( const double* )d_prev_surface, ( const double* )d_prev_stats, su,
                          ( double* )d_out_stats, ( double* )d_out_motion, c.stream );
    HIP_TRY( hipGetLastError() );
    return call_end( c );
}

extern "C" int acn_reproject( acn_scene_handle* h, const double* cur_surface, size_t n, const acn_params* prev_params, const double* prev_surface,
                              const double* prev_stats, const acn_reproject_params* prm, double* out_stats, double* out_motion,
                              const acn_render_opts* opts )
{
    Call c( opts );
    ReprojectSetup su;
    int st = reproject_check( h, cur_surface, n, prev_params, prev_surface, prev_stats, prm, out_stats, out_motion, c.opts, &su );
    if( st != ACN_OK || n == 0 ) return st;
    const size_t prev_n = ( size_t )( prev_params->image_width * prev_params->image_height );
    HostCall hc( h );
    void* d_cur = hc.in( cur_surface, sizeof( double ) * ACN_SURF_STRIDE * n );
    void* d_ps = hc.in( prev_surface, sizeof( double ) * ACN_SURF_STRIDE * prev_n );
    void* d_pt = hc.in( prev_stats, sizeof( double ) * ACN_STATS_STRIDE * prev_n );
    void* d_out = hc.out( out_stats, sizeof( double ) * ACN_STATS_STRIDE * n );
    void* d_motion = hc.out( out_motion, sizeof( double ) * 2 * n );
    c.opts.stream = nullptr;
    return hc.run( [ & ] { return acn_reproject_dev( h, d_cur, n, prev_params, d_ps, d_pt, prm, d_out, d_motion, &c.opts ); } );
}

/* ---- reprojection through moving objects (k_reproject.hip; the table's checks and acn_motion_from_scenes: acn_motion_host.h) ---- */
static int reproject_moving_check( const acn_scene_handle* h, const void* cur_surface, size_t n, const acn_params* prev_params, const void* prev_surface,
                                   const void* prev_stats, const void* motion, size_t n_motion, const acn_reproject_params* prm,
                                   const void* out_stats, const void* out_motion, const acn_render_opts& opts, ReprojectSetup* su )
{
    int st = reproject_check( h, cur_surface, n, prev_params, prev_surface, prev_stats, prm, out_stats, out_motion, opts, su );
    if( st != ACN_OK ) return st;
    std::string msg;
    if( acn_motion_table_check( motion, n_motion, n, &msg ) != ACN_OK ) return fail( ACN_ERR_ARG, msg );
    return ACN_OK;
}

extern "C" int acn_reproject_moving_dev( acn_scene_handle* h, const void* d_cur_surface, size_t n, const acn_params* prev_params,
                                         const void* d_prev_surface, const void* d_prev_stats, const void* d_motion, size_t n_motion,
                                         const acn_reproject_params* prm, void* d_out_stats, void* d_out_motion, const acn_render_opts* opts )
{
    Call c( opts );
    ReprojectSetup su;
    int st = reproject_moving_check( h, d_cur_surface, n, prev_params, d_prev_surface, d_prev_stats, d_motion, n_motion, prm, d_out_stats, d_out_motion,
                                     c.opts, &su );
    if( st != ACN_OK || n == 0 ) return st;
    if( ( st = call_begin( h, &c ) ) != ACN_OK ) return st;
    acn_launch_reproject_moving( ( const double* )d_cur_surface, n, *prev_params, ( const double* )d_prev_surface, ( const double* )d_prev_stats,
                                 ( const double* )d_motion, n_motion, su, ( double* )d_out_stats, ( double* )d_out_motion, c.stream );
    HIP_TRY( hipGetLastError() );
    return call_end( c );
}

extern "C" int acn_reproject_moving( acn_scene_handle* h, const double* cur_surface, size_t n, const acn_params* prev_params, const double* prev_surface,
                                     const double* prev_stats, const double* motion, size_t n_motion, const acn_reproject_params* prm,
                                     double* out_stats, double* out_motion, const acn_render_opts* opts )
{
    Call c( opts );
    ReprojectSetup su;
    int st = reproject_moving_check( h, cur_surface, n, prev_params, prev_surface, prev_stats, motion, n_motion, prm, out_stats, out_motion, c.opts, &su );
    if( st != ACN_OK || n == 0 ) return st;
    const size_t prev_n = ( size_t )( prev_params->image_width * prev_params->image_height );
    HostCall hc( h );
    void* d_cur = hc.in( cur_surface, sizeof( double ) * ACN_SURF_STRIDE * n );
    void* d_ps = hc.in( prev_surface, sizeof( double ) * ACN_SURF_STRIDE * prev_n );
    void* d_pt = hc.in( prev_stats, sizeof( double ) * ACN_STATS_STRIDE * prev_n );
    void* d_table = hc.in( motion, sizeof( double ) * ACN_MOTION_STRIDE * n_motion );
    void* d_out = hc.out( out_stats, sizeof( double ) * ACN_STATS_STRIDE * n );
    void* d_motion = hc.out( out_motion, sizeof( double ) * 2 * n );
    c.opts.stream = nullptr;
    return hc.run( [ & ] { return acn_reproject_moving_dev( h, d_cur, n, prev_params, d_ps, d_pt, d_table, n_motion, prm, d_out, d_motion, &c.opts ); } );
}

/* ---- shadow records and the history guard (k_shadow.hip; the checks that need no handle: acn_shadow_host.h) ---- */
extern "C" int acn_shadow_records_dev( acn_scene_handle* h, const void* d_surface, size_t n, const acn_shadow_params* prm, void* d_out,
                                       const acn_render_opts* opts )
{
    Call c( opts );
    std::string msg;
    uint32_t log2_samples = 0;
    if( acn_shadow_records_check( h != nullptr, d_surface, n, prm, d_out, c.opts.shard_world, &log2_samples, &msg ) != ACN_OK ) return fail( ACN_ERR_ARG, msg );
    if( n == 0 ) return ACN_OK;
    int st = call_begin( h, &c );
    if( st != ACN_OK ) return st;
    SceneArgs s;
    if( ( st = surface_flags_begin( h, &s ) ) != ACN_OK ) return st;
    acn_launch_shadow( h->scene.lds_bytes != 0, h->scene.leaf_lights, machine_lds_bytes( h->scene ), c.stream, s, ( const double* )d_surface, n,
                       log2_samples, ( double* )d_out );
    HIP_TRY( hipGetLastError() );
    return surface_flags_end( h, c );
}

extern "C" int acn_shadow_records( acn_scene_handle* h, const double* surface, size_t n, const acn_shadow_params* prm, double* out,
                                   const acn_render_opts* opts )
{
    Call c( opts );
    std::string msg;
    uint32_t log2_samples = 0;
    if( acn_shadow_records_check( h != nullptr, surface, n, prm, out, c.opts.shard_world, &log2_samples, &msg ) != ACN_OK ) return fail( ACN_ERR_ARG, msg );
    if( n == 0 ) return ACN_OK;
    c.opts.stream = nullptr;
    return host_in_out( h, surface, sizeof( double ) * ACN_SURF_STRIDE * n, out, sizeof( double ) * ACN_SHADOW_STRIDE * n,
                        [ & ]( void* d_in, void* d_out ) { return acn_shadow_records_dev( h, d_in, n, prm, d_out, &c.opts ); } );
}

extern "C" int acn_shadow_limit_history_dev( acn_scene_handle* h, void* d_stats, const void* d_motion, const void* d_cur_shadow, const void* d_prev_shadow,
                                             size_t n, size_t prev_width, size_t prev_height, const acn_shadow_history_params* prm, void* d_out_change,
                                             const acn_render_opts* opts )
{
    Call c( opts );
    std::string msg;
    acn_shadow_history_params p;
    if( acn_shadow_limit_history_check( h != nullptr, d_stats, d_motion, d_cur_shadow, d_prev_shadow, n, prev_width, prev_height, prm, d_out_change,
                                        c.opts.shard_world, &p, &msg ) != ACN_OK ) return fail( ACN_ERR_ARG, msg );
    if( n == 0 ) return ACN_OK;
    int st = call_begin( h, &c );
    if( st != ACN_OK ) return st;
    ShadowHistorySetup su;
    su.drop = ( p.flags & ACN_SHADOW_HISTORY_DROP ) ? 1u : 0u; su.tolerance = p.tolerance; su.cap = p.changed_max_history;
    acn_launch_shadow_limit_history( ( double* )d_stats, ( const double* )d_motion, ( const double* )d_cur_shadow, ( const double* )d_prev_shadow, n,
                                     prev_width, prev_height, su, ( double* )d_out_change, c.stream );
    HIP_TRY( hipGetLastError() );
    return call_end( c );
}

extern "C" int acn_shadow_limit_history( acn_scene_handle* h, double* stats, const double* motion, const double* cur_shadow, const double* prev_shadow,
                                         size_t n, size_t prev_width, size_t prev_height, const acn_shadow_history_params* prm, double* out_change,
                                         const acn_render_opts* opts )
{
    Call c( opts );
    std::string msg;
    acn_shadow_history_params p;
    if( acn_shadow_limit_history_check( h != nullptr, stats, motion, cur_shadow, prev_shadow, n, prev_width, prev_height, prm, out_change,
                                        c.opts.shard_world, &p, &msg ) != ACN_OK ) return fail( ACN_ERR_ARG, msg );
    if( n == 0 ) return ACN_OK;
    HostCall hc( h );
    void* d_stats = hc.inout( stats, stats, sizeof( double ) * ACN_STATS_STRIDE * n );
    void* d_motion = hc.in( motion, sizeof( double ) * 2 * n );
    void* d_cur = hc.in( cur_shadow, sizeof( double ) * ACN_SHADOW_STRIDE * n );
    void* d_prev = hc.in( prev_shadow, sizeof( double ) * ACN_SHADOW_STRIDE * prev_width * prev_height );
    void* d_change = hc.out( out_change, sizeof( double ) * n );
    c.opts.stream = nullptr;
    return hc.run( [ & ] { return acn_shadow_limit_history_dev( h, d_stats, d_motion, d_cur, d_prev, n, prev_width, prev_height, prm, d_change, &c.opts ); } );
}

extern "C" int acn_motion_from_scenes( const acn_flat_scene* prev, const acn_flat_scene* cur, double moved_max_history, double* out_table,
                                       acn_motion_report* report )
{
    std::string msg;
    const int st = acn_motion_from_scenes_impl( prev, cur, moved_max_history, out_table, report, &msg );
    return st == ACN_OK ? ACN_OK : fail( st, msg );
}

/* ---- selecting positions by a key (k_select.hip; the checks and the host arithmetic: acn_select_host.h) ---- */
extern "C" int acn_select_above_dev( acn_scene_handle* h, const void* d_key, size_t n, const acn_select_params* prm, const void* d_src_pos_xy,
                                     void* d_out_index, void* d_out_pos_xy, void* d_out_count, uint64_t* out_count, const acn_render_opts* opts )
{
    Call c( opts );
    std::string msg;
    acn_select_params p;
    if( acn_select_args_check( h != nullptr, d_key, n, prm, d_src_pos_xy, d_out_index, d_out_pos_xy, c.opts.shard_world, &p, &msg ) != ACN_OK ) return fail( ACN_ERR_ARG, msg );
    if( ( uintptr_t )d_out_count % 8 ) return fail( ACN_ERR_ARG, "d_out_count is a uint64_t: align it" );
    const uint64_t width = p.raster_width ? p.raster_width : h->dev.prm.image_width;
    if( !d_src_pos_xy && d_out_pos_xy && width == 0 ) return fail( ACN_ERR_ARG, "raster positions need a raster_width or a scene with an image_width" );
    int st = call_begin( h, &c );
    if( st != ACN_OK ) return st;
    if( n == 0 )   /* no launch */
    {
        if( d_out_count ) HIP_TRY( hipMemsetAsync( d_out_count, 0, sizeof( uint64_t ), c.stream ) );
        if( ( st = call_end( c ) ) != ACN_OK ) return st;
        if( out_count ) *out_count = 0;
        return ACN_OK;
    }
    const size_t words = ( size_t )acn_select_tiles( n ) + 1;
    if( h->d_select_tiles.grow( sizeof( unsigned long long ) * words ) ) return ACN_ERR_DEVICE;
    acn_launch_select( ( const double* )d_key, n, p.threshold, h->d_select_tiles.get(), p.capacity, ( const double* )d_src_pos_xy, width, p.raster_first,
                       ( int64_t* )d_out_index, ( double* )d_out_pos_xy, ( unsigned long long* )d_out_count, c.stream );
    HIP_TRY( hipGetLastError() );
    if( !out_count ) return call_end( c );
    /* the one synchronisation of a caller's stream */
    unsigned long long total = 0;
    HIP_TRY( hipMemcpyAsync( &total, h->d_select_tiles.get() + ( words - 1 ), sizeof( total ), hipMemcpyDeviceToHost, c.stream ) );
    HIP_TRY( hipStreamSynchronize( c.stream ) );
    *out_count = total;
    return ACN_OK;
}

extern "C" int acn_select_above( acn_scene_handle* h, const double* key, size_t n, const acn_select_params* prm, const double* src_pos_xy,
                                 int64_t* out_index, double* out_pos_xy, uint64_t* out_count )
{
    std::string msg;
    acn_select_params p;
    if( acn_select_args_check( h != nullptr, key, n, prm, src_pos_xy, out_index, out_pos_xy, 0, &p, &msg ) != ACN_OK ) return fail( ACN_ERR_ARG, msg );
    if( n == 0 ) { if( out_count ) *out_count = 0; return ACN_OK; }
    HIP_TRY( hipSetDevice( h->device ) );
    const size_t cap = ( size_t )( p.capacity < n ? p.capacity : n );   /* (no more than n are ever selected) */
    DevCopies dc;
    void* d_key = dc.make( key, sizeof( double ) * n );
    void* d_src = src_pos_xy ? dc.make( src_pos_xy, sizeof( double ) * 2 * n ) : nullptr;
    void* d_index = out_index && cap ? dc.make( nullptr, sizeof( int64_t ) * cap ) : nullptr;
    void* d_pos = out_pos_xy && cap ? dc.make( nullptr, sizeof( double ) * 2 * cap ) : nullptr;
    if( !d_key || ( src_pos_xy && !d_src ) || ( out_index && cap && !d_index ) || ( out_pos_xy && cap && !d_pos ) ) return fail( ACN_ERR_DEVICE, "device buffers of a host call" );
    acn_select_params q = p;
    q.struct_size = ( uint32_t )sizeof( q );
    q.capacity = ( d_index || d_pos ) ? cap : 0;
    uint64_t total = 0;
    int st = acn_select_above_dev( h, d_key, n, &q, d_src, d_index, d_pos, nullptr, &total, nullptr );
    const size_t wrote = ( size_t )( total < q.capacity ? total : q.capacity );
    if( st == ACN_OK && d_index && wrote ) st = DevCopies::fetch( out_index, d_index, sizeof( int64_t ) * wrote );
    if( st == ACN_OK && d_pos && wrote ) st = DevCopies::fetch( out_pos_xy, d_pos, sizeof( double ) * 2 * wrote );
    if( st == ACN_OK && out_count ) *out_count = total;
    return st;
}

extern "C" int acn_key_histogram_dev( acn_scene_handle* h, const void* d_key, size_t n, void* d_out_hist, const acn_render_opts* opts )
{
    Call c( opts );
    std::string msg;
    if( acn_key_hist_args_check( h != nullptr, d_key, n, d_out_hist, c.opts.shard_world, &msg ) != ACN_OK ) return fail( ACN_ERR_ARG, msg );
    int st = call_begin( h, &c );
    if( st != ACN_OK ) return st;
    HIP_TRY( hipMemsetAsync( d_out_hist, 0, sizeof( uint64_t ) * ACN_KEY_HIST_WORDS, c.stream ) );
    if( n ) acn_launch_key_hist( ( const double* )d_key, n, ( unsigned long long* )d_out_hist, c.stream );
    HIP_TRY( hipGetLastError() );
    return call_end( c );
}

extern "C" int acn_key_histogram( acn_scene_handle* h, const double* key, size_t n, uint64_t* out_hist )
{
    std::string msg;
    if( acn_key_hist_args_check( h != nullptr, key, n, out_hist, 0, &msg ) != ACN_OK ) return fail( ACN_ERR_ARG, msg );
    const size_t hist_bytes = sizeof( uint64_t ) * ACN_KEY_HIST_WORDS;
    return host_in_out( h, key, sizeof( double ) * n, out_hist, hist_bytes,
                        [ & ]( void* d_key, void* d_hist ) { return acn_key_histogram_dev( h, d_key, n, d_hist, nullptr ); } );
}

extern "C" double acn_key_hist_edge( uint32_t bin ) { return acn_select_hist_edge( bin ); }
extern "C" double acn_key_hist_threshold( const uint64_t* hist, uint64_t budget ) { return acn_select_hist_threshold( hist, budget ); }

/* ---- the device-resident frame (k_frame.hip; the checks and every expression: acn_frame_host.h) ---- */
/* every frame call works on the handle's own stream and waits for it */
static int frame_begin( acn_frame* f, hipStream_t* stream )
{
    HIP_TRY( hipSetDevice( f->h->device ) );
    *stream = f->h->run.stream.get();
    return ACN_OK;
}

static const long long* frame_index( const acn_frame* f ) { return f->centres ? nullptr : f->d_index.get(); }

/* the slices of the current plan, in order: body( g0, groups ) of whole groups, at most the handle's slice bound of positions each */
template< class Body >
static int frame_slices( const acn_frame* f, Body body )
{
    const uint64_t per = acn_frame_slice_groups( f->h->tun.frame_slice, f->samples );
    for( uint64_t g0 = 0; g0 < f->flagged; g0 += per )
    {
        const int st = body( g0, f->flagged - g0 < per ? f->flagged - g0 : per );
        if( st != ACN_OK ) return st;
    }
    return ACN_OK;
}

/* the entry buffers of a plan of `flagged` groups, and its positions */
static int frame_plan_entries( acn_frame* f, bool centres, uint64_t flagged, uint64_t samples, uint64_t rval, hipStream_t stream )
{
    const uint64_t entries = flagged * samples;
    if( entries && ( f->d_pos.grow( sizeof( double ) * 2 * entries ) || f->d_clr.grow( sizeof( double ) * 3 * entries ) ) ) return ACN_ERR_DEVICE;
    f->centres = centres; f->flagged = flagged; f->samples = samples;
    int st = frame_slices( f, [ & ]( uint64_t g0, uint64_t groups )
    {
        acn_launch_frame_jitter( frame_index( f ), g0 * samples, groups * samples, samples, rval, f->width, f->d_pos.get(), stream );
        HIP_TRY( hipGetLastError() );
        return ( int )ACN_OK;
    } );
    if( st == ACN_OK && entries ) HIP_TRY( hipStreamSynchronize( stream ) );
    f->planned = st == ACN_OK;
    return st;
}

static int frame_plan( acn_frame* f, double sqr_threshold, uint64_t samples, uint64_t rval, uint64_t* out_flagged, uint64_t* out_rval )
{
    std::string msg;
    if( acn_frame_plan_check( f != nullptr, f && f->planned, sqr_threshold, samples, &msg ) != ACN_OK ) return fail( ACN_ERR_ARG, msg );
    hipStream_t stream;
    int st = frame_begin( f, &stream );
    if( st != ACN_OK ) return st;
    acn_scene_handle* h = f->h;
    const uint64_t n = f->width * f->height;
    const size_t words = ( size_t )acn_select_tiles( n ) + 1;
    if( h->d_select_tiles.grow( sizeof( unsigned long long ) * words ) ) return ACN_ERR_DEVICE;
    acn_launch_frame_key( f->d_acc.get(), f->width, f->height, f->d_key.get(), stream );
    HIP_TRY( hipGetLastError() );
    acn_launch_select( f->d_key.get(), n, sqr_threshold, h->d_select_tiles.get(), n, nullptr, f->width, 0, ( int64_t* )f->d_index.get(), nullptr, nullptr, stream );
    HIP_TRY( hipGetLastError() );
    unsigned long long flagged = 0;
    HIP_TRY( hipMemcpyAsync( &flagged, h->d_select_tiles.get() + ( words - 1 ), sizeof( flagged ), hipMemcpyDeviceToHost, stream ) );
    HIP_TRY( hipStreamSynchronize( stream ) );
    if( ( st = frame_plan_entries( f, false, flagged, samples, rval, stream ) ) != ACN_OK ) return st;
    if( out_flagged ) *out_flagged = flagged;
    if( out_rval ) *out_rval = acn_frame_lcg00_jump( rval, 2 * samples * flagged );
    return ACN_OK;
}

static int frame_render( acn_frame* f, const Call& c )
{
    std::string msg;
    if( acn_frame_step_check( f != nullptr, f && f->planned, "render", c.opts.shard_world, f ? f->width : 0, f ? f->height : 0,
                              f ? f->h->dev.prm.image_width : 0, f ? f->h->dev.prm.image_height : 0, true, &msg ) != ACN_OK ) return fail( ACN_ERR_ARG, msg );
    hipStream_t stream;
    int st = frame_begin( f, &stream );
    if( st != ACN_OK ) return st;
    acn_render_opts opts = c.opts;
    opts.stream = nullptr;
    st = frame_slices( f, [ & ]( uint64_t g0, uint64_t groups )
    {
        const uint64_t e0 = g0 * f->samples;
        return render_dispatch( f->h, primary_positions( f->d_pos.get() + 2 * e0 ), ( size_t )( groups * f->samples ), f->d_clr.get() + 3 * e0, &opts, stream );
    } );
    if( st == ACN_OK ) HIP_TRY( hipStreamSynchronize( stream ) );
    return st;
}

static int frame_push( acn_frame* f )
{
    std::string msg;
    if( acn_frame_step_check( f != nullptr, f && f->planned, "push", 0, 0, 0, 0, 0, false, &msg ) != ACN_OK ) return fail( ACN_ERR_ARG, msg );
    hipStream_t stream;
    int st = frame_begin( f, &stream );
    if( st != ACN_OK ) return st;
    f->planned = false;   /* consumed, whatever happens now */
    const uint64_t entries = f->flagged * f->samples;
    if( entries == 0 ) return ACN_OK;
    const uint32_t slots = f->h->tun.frame_foreign_slots;
    if( !f->centres )   /* (a pixel centre has no foreign target) */
    {
        if( f->d_foreign.grow( sizeof( unsigned long long ) * ( 1 + ( size_t )slots ) ) ) return ACN_ERR_DEVICE;
        acn_launch_frame_foreign( frame_index( f ), f->d_pos.get(), f->d_clr.get(), entries, f->samples, f->width, f->height, slots, f->d_foreign.get(),
                                  f->d_acc.get(), stream );
        HIP_TRY( hipGetLastError() );
    }
    st = frame_slices( f, [ & ]( uint64_t g0, uint64_t groups )
    {
        acn_launch_frame_push( frame_index( f ), f->d_pos.get(), f->d_clr.get(), g0, groups, f->samples, f->width, f->height, f->d_acc.get(), stream );
        HIP_TRY( hipGetLastError() );
        return ( int )ACN_OK;
    } );
    if( st != ACN_OK ) return st;
    HIP_TRY( hipStreamSynchronize( stream ) );
    return ACN_OK;
}

extern "C" int acn_frame_create( acn_scene_handle* h, uint64_t width, uint64_t height, acn_frame** out )
{
    std::string msg;
    if( acn_frame_create_check( h != nullptr, width, height, out, &msg ) != ACN_OK ) return fail( ACN_ERR_ARG, msg );
    HIP_TRY( hipSetDevice( h->device ) );
    std::unique_ptr< acn_frame > f( new acn_frame );
    f->h = h; f->width = width; f->height = height;
    const size_t n = ( size_t )( width * height );
    if( f->d_acc.grow( sizeof( double ) * 6 * n ) || f->d_key.grow( sizeof( double ) * n ) || f->d_index.grow( sizeof( long long ) * n ) ) return ACN_ERR_DEVICE;
    HIP_TRY( hipMemsetAsync( f->d_acc.get(), 0, sizeof( double ) * 6 * n, h->run.stream.get() ) );
    HIP_TRY( hipStreamSynchronize( h->run.stream.get() ) );
    *out = f.get();
    h->frames.push_back( std::move( f ) );
    return ACN_OK;
}

extern "C" void acn_frame_free( acn_frame* f )
{
    if( !f ) return;
    acn_scene_handle* h = f->h;
    hipSetDevice( h->device );
    for( size_t i = 0; i < h->frames.size(); i++ )
        if( h->frames[ i ].get() == f ) { h->frames.erase( h->frames.begin() + ( long )i ); return; }
}

extern "C" int acn_frame_upload( acn_frame* f, const double* lum )
{
    std::string msg;
    if( acn_frame_copy_check( f != nullptr, lum, &msg ) != ACN_OK ) return fail( ACN_ERR_ARG, msg );
    hipStream_t stream;
    int st = frame_begin( f, &stream );
    if( st != ACN_OK ) return st;
    f->planned = false;
    HIP_TRY( hipMemcpy( f->d_acc.get(), lum, sizeof( double ) * 6 * f->width * f->height, hipMemcpyHostToDevice ) );
    return ACN_OK;
}

extern "C" int acn_frame_download( acn_frame* f, double* lum )
{
    std::string msg;
    if( acn_frame_copy_check( f != nullptr, lum, &msg ) != ACN_OK ) return fail( ACN_ERR_ARG, msg );
    hipStream_t stream;
    int st = frame_begin( f, &stream );
    if( st != ACN_OK ) return st;
    HIP_TRY( hipMemcpy( lum, f->d_acc.get(), sizeof( double ) * 6 * f->width * f->height, hipMemcpyDeviceToHost ) );
    return ACN_OK;
}

extern "C" int acn_frame_plan( acn_frame* f, double sqr_threshold, uint64_t samples, uint64_t rval, uint64_t* out_flagged, uint64_t* out_rval )
{
    return frame_plan( f, sqr_threshold, samples, rval, out_flagged, out_rval );
}

extern "C" int acn_frame_render( acn_frame* f, const acn_render_opts* opts )
{
    Call c( opts );
    return frame_render( f, c );
}

extern "C" int acn_frame_push( acn_frame* f ) { return frame_push( f ); }

/* render, the cancel flag once more, push; a pass that does not get to its push drops its plan */
static int frame_render_push( acn_frame* f, const Call& c )
{
    int st = frame_render( f, c );
    if( st == ACN_OK && c.opts.cancel && *c.opts.cancel ) st = fail( ACN_ERR_CANCELLED, "cancelled" );
    if( st != ACN_OK ) { f->planned = false; return st; }
    return frame_push( f );
}

extern "C" int acn_frame_main_pass( acn_frame* f, const acn_render_opts* opts )
{
    Call c( opts );
    std::string msg;
    if( acn_frame_plan_check( f != nullptr, f && f->planned, 0.0, 1, &msg ) != ACN_OK ) return fail( ACN_ERR_ARG, msg );
    if( acn_frame_step_check( true, true, "render", c.opts.shard_world, f->width, f->height, f->h->dev.prm.image_width, f->h->dev.prm.image_height, true,
                              &msg ) != ACN_OK ) return fail( ACN_ERR_ARG, msg );
    hipStream_t stream;
    int st = frame_begin( f, &stream );
    if( st != ACN_OK ) return st;
    if( ( st = frame_plan_entries( f, true, f->width * f->height, 1, 0, stream ) ) != ACN_OK ) return st;
    return frame_render_push( f, c );
}

extern "C" int acn_frame_pass( acn_frame* f, double sqr_threshold, uint64_t samples, uint64_t* rval, uint64_t* out_flagged, const acn_render_opts* opts )
{
    Call c( opts );
    std::string msg;
    if( acn_frame_pass_check( f != nullptr, rval, &msg ) != ACN_OK ) return fail( ACN_ERR_ARG, msg );
    if( acn_frame_plan_check( true, f->planned, sqr_threshold, samples, &msg ) != ACN_OK ) return fail( ACN_ERR_ARG, msg );
    if( acn_frame_step_check( true, true, "render", c.opts.shard_world, f->width, f->height, f->h->dev.prm.image_width, f->h->dev.prm.image_height, true,
                              &msg ) != ACN_OK ) return fail( ACN_ERR_ARG, msg );
    uint64_t flagged = 0, next = 0;
    int st = frame_plan( f, sqr_threshold, samples, *rval, &flagged, &next );
    if( st != ACN_OK ) return st;
    if( ( st = frame_render_push( f, c ) ) != ACN_OK ) return st;
    *rval = next;
    if( out_flagged ) *out_flagged = flagged;
    return ACN_OK;
}

extern "C" int acn_frame_image( acn_frame* f, double* out_rgb, uint8_t* out_rgb8 )
{
    if( !f ) return fail( ACN_ERR_ARG, "null argument: frame" );
    if( !out_rgb && !out_rgb8 ) return ACN_OK;
    hipStream_t stream;
    int st = frame_begin( f, &stream );
    if( st != ACN_OK ) return st;
    const size_t n = ( size_t )( f->width * f->height ), rgb_bytes = sizeof( double ) * 3 * n;
    if( f->d_image.grow( rgb_bytes + 3 * n ) ) return ACN_ERR_DEVICE;
    double* d_rgb = ( double* )f->d_image.get();
    unsigned char* d_rgb8 = ( unsigned char* )f->d_image.get() + rgb_bytes;
    acn_launch_frame_image( f->d_acc.get(), n, out_rgb ? d_rgb : nullptr, out_rgb8 ? d_rgb8 : nullptr, stream );
    HIP_TRY( hipGetLastError() );
    if( out_rgb ) HIP_TRY( hipMemcpyAsync( out_rgb, d_rgb, rgb_bytes, hipMemcpyDeviceToHost, stream ) );
    if( out_rgb8 ) HIP_TRY( hipMemcpyAsync( out_rgb8, d_rgb8, 3 * n, hipMemcpyDeviceToHost, stream ) );
    HIP_TRY( hipStreamSynchronize( stream ) );
    return ACN_OK;
}

extern "C" int acn_frame_view( acn_frame* f, acn_frame_buffers* out )
{
    std::string msg;
    if( acn_frame_view_check( f != nullptr, out, &msg ) != ACN_OK ) return fail( ACN_ERR_ARG, msg );
    acn_frame_buffers b{};
    b.struct_size = out->struct_size < sizeof( b ) ? out->struct_size : ( uint32_t )sizeof( b );
    b.planned = f->planned ? 1u : 0u;
    b.width = f->width; b.height = f->height;
    b.flagged = f->planned ? f->flagged : 0; b.samples = f->planned ? f->samples : 0;
    b.d_accumulator = f->d_acc.get(); b.d_key = f->d_key.get(); b.d_index = f->d_index.get();
    b.d_positions = f->d_pos.get(); b.d_colours = f->d_clr.get();
    memcpy( out, &b, b.struct_size );
    return ACN_OK;
}

extern "C" uint64_t acn_lcg00_jump( uint64_t rval, uint64_t draws ) { return acn_frame_lcg00_jump( rval, draws ); }

/* ---- test seams: the envelope estimate and the deterministic math library, on the device's arithmetic ---- */
extern "C" int acn_estimate_envelope( acn_scene_handle* h, int32_t node, uint64_t samples, uint32_t rseed,
                                      double radius_factor, double* out )
{
    Call c( nullptr );
    if( !h || !out || node < 0 || ( uint32_t )node >= h->dev.n_nodes ) return fail( ACN_ERR_ARG, "bad argument" );
    int st = call_begin( h, &c );
    if( st != ACN_OK ) return st;
    DevCopies dc;
    void* d_scratch = dc.make( nullptr, sizeof( V3 ) * ( samples ? samples : 1 ) );
    void* d_out = dc.make( nullptr, sizeof( double ) * 4 );
    if( !d_scratch || !d_out ) return fail( ACN_ERR_DEVICE, "device buffers of a host call" );
    DevScene est_scene = h->dev;
    est_scene.lds_stack = ACN_NO_LDS_STACK;   /* one lane, no dynamic LDS: the machine keeps its stacks in scratch */
    hipLaunchKernelGGL( k_estimate_envelope, dim3( 1 ), dim3( 1 ), 0, c.stream, est_scene, node, samples, rseed, radius_factor, ( V3* )d_scratch, ( double* )d_out );
    HIP_TRY( hipGetLastError() );
    st = call_end( c );
    return st != ACN_OK ? st : DevCopies::fetch( out, d_out, sizeof( double ) * 4 );
}

extern "C" int acn_detmath_eval( int device, int op, const double* x, const double* y, double* out, size_t n )
{
    if( !x || !out ) return fail( ACN_ERR_ARG, "null argument" );
    if( acn_device_count() <= 0 ) return fail( ACN_ERR_DEVICE, "no HIP device" );
    HIP_TRY( hipSetDevice( device ) );
    DevCopies dc;
    void* dx = dc.make( x, sizeof( double ) * n );
    void* dout = dc.make( nullptr, sizeof( double ) * n );
    void* dy = y ? dc.make( y, sizeof( double ) * n ) : nullptr;
    if( !dx || !dout || ( y && !dy ) ) return fail( ACN_ERR_DEVICE, "device buffers of a host call" );
    hipLaunchKernelGGL( k_detmath, dim3( ( unsigned )( ( n + 255 ) / 256 ) ), dim3( 256 ), 0, 0, op, ( const double* )dx, ( const double* )dy, ( double* )dout, n );
    HIP_TRY( hipGetLastError() );
    HIP_TRY( hipDeviceSynchronize() );
    return DevCopies::fetch( out, dout, sizeof( double ) * n );
}
