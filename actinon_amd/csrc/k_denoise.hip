/* k_denoise.hip -- the edge-avoiding a-trous filter of acn_denoise (include/actinon_hip.h states every expression and its order;
 * tests/denoise_model.py restates them in numpy and the two are compared bit for bit).
 *
 * The steps that the layered filter (k_denoise_layers.hip) takes too have their one body in acn_denoise_dev.h: dn_guide, dn_prefilter,
 * dn_level.  The kernels here run the two window bodies on the pixels themselves (DnPixelSource) and keep what is their own.
 * Launches of one call: k_dn_prepare, k_dn_variance, k_dn_level once per level; the last level remodulates and writes the frame.
 *   prepare   one pixel per lane: dn_guide reads the lane's 128-byte surface record with 16-byte loads (the line k_surface wrote
 *             whole) and writes what a tap needs as two aligned pieces: a 64-byte guide (N, P, the match key) and 32 bytes { c.xyz, var }.
 *   variance  7 x 7 window on the guide keys and the colours.
 *   level     dn_level: 5 x 5 taps at stride 2^i, a gather: per tap 16 bytes of key, then 48 bytes of N, P and 32 bytes of colour.
 *             The kernel adds the copy of the pixels that are not filterable and the remodulation of the last level.
 * The window kernels run 256-lane workgroups on 16 x 16 pixel tiles, lane t on pixel ( t & 15, t >> 4 ) of the tile: a wave covers
 * 16 x 4 pixels, so the 25 taps of a wave fall on few lines.  Tiles are numbered in one grid dimension (an image 1 pixel wide and
 * 2^31 high has more rows of tiles than a grid has in y).  A tap that is skipped is predicated: its address is clamped to the
 * centre, it is loaded, and a select drops its terms -- sums start at +0 and never become -0, so adding the +0 of a dropped term
 * is adding nothing.  The one branch is wave-level: a tap that no lane of the wave takes (most of them at stride 64 near a border)
 * is not loaded, which for the same reason changes no bit.  No lane reads another lane's registers.
 *
 * acn_denoise_stats (frames of acn_render_lens_stats*) launches k_dn_prepare_stats, k_dn_prefilter and the same k_dn_level:
 *   prepare_stats  also reads the lane's 64-byte statistics record with 16-byte loads; the colour piece is { c.xyz, var_raw }, a
 *                  negative var_raw standing for "none", and the pixel's mean (the background for an EMPTY record) goes to the
 *                  frame, where the last level finds the pixels it copies.
 *   prefilter      dn_prefilter: 3 x 3 window on the guide keys and var_raw, in the arrangement of `variance`.
 * dn_launch_levels launches the levels of either call. */
#include <hip/hip_runtime.h>
#include "acn_launch.h"
#include "acn_denoise_dev.h"

__global__ __launch_bounds__( 256 )
void k_dn_prepare( const double* __restrict__ lin, const double* __restrict__ surf, size_t n, uint32_t no_demodulate,
                   double2* __restrict__ guide, double2* __restrict__ pix )
{
    const size_t i = ( size_t )blockIdx.x * blockDim.x + threadIdx.x;
    if( i >= n ) return;
    const double2 none = make_double2( 0.0, 0.0 );
    dn_guide< false >( surf, i, no_demodulate, true, lin[ 3 * i ], lin[ 3 * i + 1 ], lin[ 3 * i + 2 ], none, none, none, guide, pix );
}

__global__ __launch_bounds__( 256 )
void k_dn_variance( const double2* __restrict__ guide, const double2* __restrict__ in, size_t width, size_t height, size_t tiles_x,
                    double2* __restrict__ out )
{
    size_t x, y;
    if( !dn_pixel( width, height, tiles_x, &x, &y ) ) return;
    const size_t p = y * width + x;
    const DnKey key = dn_key( guide, p );
    const double2 c0 = in[ 2 * p ], c1 = in[ 2 * p + 1 ];
    double var = 0.0;
    if( key.ok )
    {
        double n = 0.0, s1 = 0.0, s2 = 0.0;
        #pragma unroll 1
        for( int dy = -3; dy <= 3; dy++ )
        {
            #pragma unroll
            for( int dx = -3; dx <= 3; dx++ )
            {
                bool inside;
                const size_t q = dn_tap( x, y, dx, dy, width, height, p, &inside );
                const DnKey k2 = dn_key( guide, q );
                const bool ok = inside && dn_match( key, k2 );
                const double2 t0 = in[ 2 * q ];
                const double tz = in[ 2 * q + 1 ].x;
                const double l = dn_lum( t0.x, t0.y, tz );
                n  += ok ? 1.0 : 0.0;
                s1 += ok ? l : 0.0;
                s2 += ok ? l * l : 0.0;
            }
        }
        const double m = s1 / n;
        const double v = s2 / n - m * m;
        var = v > 0 ? v : 0.0;
    }
    out[ 2 * p ]     = c0;
    out[ 2 * p + 1 ] = make_double2( c1.x, var );
}

/* steps 1 and 2 of acn_denoise_stats: L is the mean of the record, var_raw the measured variance of the demodulated mean */
__global__ __launch_bounds__( 256 )
void k_dn_prepare_stats( const double2* __restrict__ stats, const double* __restrict__ surf, size_t n, uint32_t no_demodulate,
                         double bg_x, double bg_y, double bg_z, double2* __restrict__ guide, double2* __restrict__ pix, double* __restrict__ frame )
{
    const size_t i = ( size_t )blockIdx.x * blockDim.x + threadIdx.x;
    if( i >= n ) return;
    const double2 s0 = stats[ 4 * i ], s1 = stats[ 4 * i + 1 ], s2 = stats[ 4 * i + 2 ], s3 = stats[ 4 * i + 3 ];
    const bool empty = stats_empty( s0.x );
    const double lx = empty ? bg_x : s0.y, ly = empty ? bg_y : s1.x, lz = empty ? bg_z : s1.y;
    dn_guide< true >( surf, i, no_demodulate, !empty, lx, ly, lz, s0, s2, s3, guide, pix );
    frame[ 3 * i ] = lx; frame[ 3 * i + 1 ] = ly; frame[ 3 * i + 2 ] = lz;
}

/* dn_prefilter over the pixels themselves, in the arrangement of `variance` */
__global__ __launch_bounds__( 256 )
void k_dn_prefilter( const double2* __restrict__ guide, const double2* __restrict__ in, size_t width, size_t height, size_t tiles_x,
                     double2* __restrict__ out )
{
    size_t x, y;
    if( !dn_pixel( width, height, tiles_x, &x, &y ) ) return;
    const size_t p = y * width + x;
    const double2 c0 = in[ 2 * p ], c1 = in[ 2 * p + 1 ];
    const double var = dn_prefilter( DnPixelSource(), guide, in, x, y, p, dn_key( guide, p ), width, height );
    out[ 2 * p ]     = c0;
    out[ 2 * p + 1 ] = make_double2( c1.x, var );
}

/* one a-trous level.  LAST: the result is remodulated and written to the frame, pixels that are not filterable are copied there */
template< bool LAST >
__global__ __launch_bounds__( 256 )
void k_dn_level( const double2* __restrict__ guide, const double2* __restrict__ in, size_t width, size_t height, size_t tiles_x,
                 long long stride, uint32_t normal_power_log2, double sigma_plane, double sigma_lum, double2* __restrict__ out,
                 const double* lin, const double* __restrict__ surf, uint32_t no_demodulate, double* out_rgb )
{
    size_t x, y;
    if( !dn_pixel( width, height, tiles_x, &x, &y ) ) return;
    const size_t p = y * width + x;
    const DnKey key = dn_key( guide, p );
    if( !key.ok )
    {
        if constexpr( LAST )
        {
            const double a = lin[ 3 * p ], b = lin[ 3 * p + 1 ], c = lin[ 3 * p + 2 ];   /* (in place: this lane alone touches the pixel) */
            out_rgb[ 3 * p ] = a; out_rgb[ 3 * p + 1 ] = b; out_rgb[ 3 * p + 2 ] = c;
        }
        return;
    }
    double2 o0, o1;
    dn_level( DnPixelSource(), guide, in, x, y, p, p, key, width, height, stride, normal_power_log2, sigma_plane, sigma_lum, &o0, &o1 );
    if constexpr( LAST )
    {
        const double2* r = ( const double2* )( surf + ( size_t )ACN_SURF_STRIDE * p );
        const double2 r4 = r[ 4 ], r5 = r[ 5 ];
        out_rgb[ 3 * p ]     = o0.x * dn_albedo( r4.y, no_demodulate );
        out_rgb[ 3 * p + 1 ] = o0.y * dn_albedo( r5.x, no_demodulate );
        out_rgb[ 3 * p + 2 ] = o1.x * dn_albedo( r5.y, no_demodulate );
    }
    else { out[ 2 * p ] = o0; out[ 2 * p + 1 ] = o1; }
}

/* the levels of one call: they ping-pong between buf[ 1 ] and buf[ 0 ]; the last one remodulates, writes the frame and copies the
 * pixels that are not filterable from `copies` */
static void dn_launch_levels( const double2* guide, double2* const* buf, dim3 tiles, size_t width, size_t height, size_t tiles_x, uint32_t iterations,
                              uint32_t normal_power_log2, double sigma_plane, double sigma_lum, const double* copies, const double* surf,
                              uint32_t no_demodulate, double* out_rgb, hipStream_t stream )
{
    int src = 1;
    for( uint32_t i = 0; i < iterations; i++, src ^= 1 )
    {
        const long long stride = 1ll << i;
        if( i + 1 < iterations )
            hipLaunchKernelGGL( ( k_dn_level< false > ), tiles, dim3( 256 ), 0, stream, guide, buf[ src ], width, height, tiles_x, stride,
                                normal_power_log2, sigma_plane, sigma_lum, buf[ src ^ 1 ], ( const double* )nullptr, ( const double* )nullptr, 0u, ( double* )nullptr );
        else
            hipLaunchKernelGGL( ( k_dn_level< true > ), tiles, dim3( 256 ), 0, stream, guide, buf[ src ], width, height, tiles_x, stride,
                                normal_power_log2, sigma_plane, sigma_lum, ( double2* )nullptr, copies, surf, no_demodulate, out_rgb );
    }
}

/* scratch: [ n ] guides of 64 bytes, then two colour buffers [ n ] of 32 bytes (ACN_DENOISE_SCRATCH_PER_PIXEL in all) */
void acn_launch_denoise( const double* lin, const double* surf, size_t width, size_t height, uint32_t iterations, uint32_t normal_power_log2,
                         uint32_t no_demodulate, double sigma_plane, double sigma_lum, void* scratch, double* out_rgb, hipStream_t stream )
{
    const size_t n = width * height;
    double2* guide = ( double2* )scratch;
    double2* buf[ 2 ] = { guide + 4 * n, guide + 6 * n };
    const size_t tiles_x = ( width + DN_TILE - 1 ) / DN_TILE, tiles_y = ( height + DN_TILE - 1 ) / DN_TILE;
    const dim3 tiles( ( unsigned )( tiles_x * tiles_y ) );   /* n <= 2^31: at most 2^27 + 2^23 tiles */
    hipLaunchKernelGGL( k_dn_prepare, dim3( ( unsigned )( ( n + 255 ) / 256 ) ), dim3( 256 ), 0, stream, lin, surf, n, no_demodulate, guide, buf[ 0 ] );
    hipLaunchKernelGGL( k_dn_variance, tiles, dim3( 256 ), 0, stream, guide, buf[ 0 ], width, height, tiles_x, buf[ 1 ] );
    dn_launch_levels( guide, buf, tiles, width, height, tiles_x, iterations, normal_power_log2, sigma_plane, sigma_lum, lin, surf, no_demodulate, out_rgb, stream );
}

/* acn_denoise_stats: the same scratch; the frame itself holds the per-pixel means from prepare on, which is where the last level reads
 * the pixels it copies (in place: a lane touches its own pixel alone) */
void acn_launch_denoise_stats( const double* stats, const double* surf, size_t width, size_t height, uint32_t iterations, uint32_t normal_power_log2,
                               uint32_t no_demodulate, double sigma_plane, double sigma_lum, const double* background, void* scratch,
                               double* out_rgb, hipStream_t stream )
{
    const size_t n = width * height;
    double2* guide = ( double2* )scratch;
    double2* buf[ 2 ] = { guide + 4 * n, guide + 6 * n };
    const size_t tiles_x = ( width + DN_TILE - 1 ) / DN_TILE, tiles_y = ( height + DN_TILE - 1 ) / DN_TILE;
    const dim3 tiles( ( unsigned )( tiles_x * tiles_y ) );
    hipLaunchKernelGGL( k_dn_prepare_stats, dim3( ( unsigned )( ( n + 255 ) / 256 ) ), dim3( 256 ), 0, stream, ( const double2* )stats, surf, n,
                        no_demodulate, background[ 0 ], background[ 1 ], background[ 2 ], guide, buf[ 0 ], out_rgb );
    hipLaunchKernelGGL( k_dn_prefilter, tiles, dim3( 256 ), 0, stream, guide, buf[ 0 ], width, height, tiles_x, buf[ 1 ] );
    dn_launch_levels( guide, buf, tiles, width, height, tiles_x, iterations, normal_power_log2, sigma_plane, sigma_lum, out_rgb, surf, no_demodulate, out_rgb, stream );
}
