/* k_denoise.hip -- the edge-avoiding a-trous filter of acn_denoise (include/actinon_hip.h states every expression and its order;
 * tests/denoise_model.py restates them in numpy and the two are compared bit for bit).
 *
 * Launches of one call: k_dn_prepare, k_dn_variance, k_dn_level once per level; the last level remodulates and writes the frame.
 *   prepare   one pixel per lane: reads the lane's 128-byte surface record with 16-byte loads (the line k_surface wrote whole) and
 *             writes what a tap needs as two aligned pieces: a 64-byte guide (N, P, the match key) and 32 bytes { c.xyz, var }.
 *   variance  7 x 7 window on the guide keys and the colours.
 *   level     5 x 5 taps at stride 2^i, a gather: per tap 16 bytes of key, then 48 bytes of N, P and 32 bytes of colour.
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
 *   prefilter      3 x 3 window on the guide keys and var_raw, in the arrangement of `variance`. */
#include <hip/hip_runtime.h>
#include "acn_launch.h"
#include "acn_denoise_dev.h"

__global__ __launch_bounds__( 256 )
void k_dn_prepare( const double* __restrict__ lin, const double* __restrict__ surf, size_t n, uint32_t no_demodulate,
                   double2* __restrict__ guide, double2* __restrict__ pix )
{
    const size_t i = ( size_t )blockIdx.x * blockDim.x + threadIdx.x;
    if( i >= n ) return;
    const double2* r = ( const double2* )( surf + ( size_t )ACN_SURF_STRIDE * i );
    const double2 r0 = r[ 0 ], r1 = r[ 1 ], r2 = r[ 2 ], r3 = r[ 3 ], r4 = r[ 4 ], r5 = r[ 5 ], r6 = r[ 6 ];
    const double cx = lin[ 3 * i ]     / dn_albedo( r4.y, no_demodulate );
    const double cy = lin[ 3 * i + 1 ] / dn_albedo( r5.x, no_demodulate );
    const double cz = lin[ 3 * i + 2 ] / dn_albedo( r5.y, no_demodulate );
    DnKey key;
    key.enter = ( int32_t )r3.y; key.exit = ( int32_t )r4.x; key.hops = ( int32_t )r6.y;
    key.ok = r0.x < __builtin_inf() && !( ( uint32_t )( int32_t )r6.x & ACN_SURF_EMITTER ) && dn_finite( cx ) && dn_finite( cy ) && dn_finite( cz );
    union { DnKey k; double2 d; } kv; kv.k = key;
    double2* g = guide + 4 * i;
    g[ 0 ] = make_double2( r2.x, r2.y );   /* N */
    g[ 1 ] = make_double2( r3.x, r0.y );   /* N.z, P.x */
    g[ 2 ] = make_double2( r1.x, r1.y );   /* P.y, P.z */
    g[ 3 ] = kv.d;
    pix[ 2 * i ]     = make_double2( cx, cy );
    pix[ 2 * i + 1 ] = make_double2( cz, 0.0 );
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
                const bool ok = inside && k2.ok && k2.enter == key.enter && k2.exit == key.exit && k2.hops == key.hops;
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
    const double2* r = ( const double2* )( surf + ( size_t )ACN_SURF_STRIDE * i );
    const double2 r0 = r[ 0 ], r1 = r[ 1 ], r2 = r[ 2 ], r3 = r[ 3 ], r4 = r[ 4 ], r5 = r[ 5 ], r6 = r[ 6 ];
    const double cnt = s0.x;
    const bool empty = !( cnt >= 1.0 && cnt < __builtin_inf() );
    const double lx = empty ? bg_x : s0.y, ly = empty ? bg_y : s1.x, lz = empty ? bg_z : s1.y;
    const double ax = dn_albedo( r4.y, no_demodulate ), ay = dn_albedo( r5.x, no_demodulate ), az = dn_albedo( r5.y, no_demodulate );
    const double cx = lx / ax, cy = ly / ay, cz = lz / az;
    DnKey key;
    key.enter = ( int32_t )r3.y; key.exit = ( int32_t )r4.x; key.hops = ( int32_t )r6.y;
    key.ok = !empty && r0.x < __builtin_inf() && !( ( uint32_t )( int32_t )r6.x & ACN_SURF_EMITTER ) && dn_finite( cx ) && dn_finite( cy ) && dn_finite( cz );
    double var_raw = -1.0;
    if( !empty && cnt > 1.0 )
    {
        const double vx = ( s2.x / ( cnt - 1.0 ) ) / cnt, vy = ( s2.y / ( cnt - 1.0 ) ) / cnt, vz = ( s3.x / ( cnt - 1.0 ) ) / cnt;
        var_raw = ( ( 0.2126 * 0.2126 ) * ( vx / ( ax * ax ) ) + ( 0.7152 * 0.7152 ) * ( vy / ( ay * ay ) ) ) + ( 0.0722 * 0.0722 ) * ( vz / ( az * az ) );
    }
    union { DnKey k; double2 d; } kv; kv.k = key;
    double2* g = guide + 4 * i;
    g[ 0 ] = make_double2( r2.x, r2.y );   /* N */
    g[ 1 ] = make_double2( r3.x, r0.y );   /* N.z, P.x */
    g[ 2 ] = make_double2( r1.x, r1.y );   /* P.y, P.z */
    g[ 3 ] = kv.d;
    pix[ 2 * i ]     = make_double2( cx, cy );
    pix[ 2 * i + 1 ] = make_double2( cz, var_raw );
    frame[ 3 * i ] = lx; frame[ 3 * i + 1 ] = ly; frame[ 3 * i + 2 ] = lz;
}

/* var = the ( 1/4, 1/2, 1/4 )^2 mean of the var_raw that the matching pixels of the 3 x 3 window have; 0 where none has one */
__global__ __launch_bounds__( 256 )
void k_dn_prefilter( const double2* __restrict__ guide, const double2* __restrict__ in, size_t width, size_t height, size_t tiles_x,
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
        double sw = 0.0, sv = 0.0;
        #pragma unroll
        for( int dy = -1; dy <= 1; dy++ )
        {
            #pragma unroll
            for( int dx = -1; dx <= 1; dx++ )
            {
                bool inside;
                const size_t q = dn_tap( x, y, dx, dy, width, height, p, &inside );
                const DnKey k2 = dn_key( guide, q );
                const double vr = in[ 2 * q + 1 ].y;
                const bool ok = inside && k2.ok && k2.enter == key.enter && k2.exit == key.exit && k2.hops == key.hops && !( vr < 0.0 );
                const double g = ( dy ? 0.25 : 0.5 ) * ( dx ? 0.25 : 0.5 );
                sw += ok ? g : 0.0;
                sv += ok ? g * vr : 0.0;
            }
        }
        var = sw > 0 ? sv / sw : 0.0;
    }
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
    const double2 g0 = guide[ 4 * p ], g1 = guide[ 4 * p + 1 ], g2 = guide[ 4 * p + 2 ];
    const double nx = g0.x, ny = g0.y, nz = g1.x, px = g1.y, py = g2.x, pz = g2.y;
    const double2 c0 = in[ 2 * p ], c1 = in[ 2 * p + 1 ];
    const double l = dn_lum( c0.x, c0.y, c1.x );
    const double den = sigma_lum * acn_sqrt( c1.y ) + 1e-8;
    double sw = 0.0, sx = 0.0, sy = 0.0, sz = 0.0, sv = 0.0;
    #pragma unroll 1
    for( int tj = 0; tj < 5; tj++ )
    {
        #pragma unroll
        for( int ti = 0; ti < 5; ti++ )
        {
            const bool centre = tj == 2 && ti == 2;
            bool inside;
            const size_t q = dn_tap( x, y, ( ti - 2 ) * stride, ( tj - 2 ) * stride, width, height, p, &inside );
            const DnKey k2 = dn_key( guide, q );
            const bool ok = inside && k2.ok && k2.enter == key.enter && k2.exit == key.exit && k2.hops == key.hops;
            if( !__any( ok ) ) continue;   /* wave-level: no lane takes this tap */
            const double2 h0 = guide[ 4 * q ], h1 = guide[ 4 * q + 1 ], h2 = guide[ 4 * q + 2 ];
            const double2 t0 = in[ 2 * q ], t1 = in[ 2 * q + 1 ];
            double wn = dn_dot( nx, ny, nz, h0.x, h0.y, h1.x );
            wn = wn > 0 ? wn : 0.0;
            for( uint32_t k = 0; k < normal_power_log2; k++ ) wn = wn * wn;
            const double dx = h1.y - px, dy = h2.x - py, dz = h2.y - pz;
            const double len = acn_sqrt( dn_dot( dx, dy, dz, dx, dy, dz ) );
            const double tp = len > 0 ? ( acn_fabs( dn_dot( nx, ny, nz, dx, dy, dz ) ) / len ) / sigma_plane : 0.0;
            const double tl = acn_fabs( dn_lum( t0.x, t0.y, t1.x ) - l ) / den;
            double w = ( ( dn_k( tj ) * dn_k( ti ) ) * wn ) * acn_exp( -( tp + tl ) );
            if( centre ) w = 0.375 * 0.375;
            sw += ok ? w : 0.0;
            sx += ok ? w * ( t0.x - c0.x ) : 0.0;
            sy += ok ? w * ( t0.y - c0.y ) : 0.0;
            sz += ok ? w * ( t1.x - c1.x ) : 0.0;
            sv += ok ? ( w * w ) * t1.y : 0.0;
        }
    }
    const double ox = c0.x + sx / sw, oy = c0.y + sy / sw, oz = c1.x + sz / sw, ov = sv / ( sw * sw );
    if constexpr( LAST )
    {
        const double2* r = ( const double2* )( surf + ( size_t )ACN_SURF_STRIDE * p );
        const double2 r4 = r[ 4 ], r5 = r[ 5 ];
        out_rgb[ 3 * p ]     = ox * dn_albedo( r4.y, no_demodulate );
        out_rgb[ 3 * p + 1 ] = oy * dn_albedo( r5.x, no_demodulate );
        out_rgb[ 3 * p + 2 ] = oz * dn_albedo( r5.y, no_demodulate );
    }
    else
    {
        out[ 2 * p ]     = make_double2( ox, oy );
        out[ 2 * p + 1 ] = make_double2( oz, ov );
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
    int src = 1;
    for( uint32_t i = 0; i < iterations; i++, src ^= 1 )
    {
        const long long stride = 1ll << i;
        if( i + 1 < iterations )
            hipLaunchKernelGGL( ( k_dn_level< false > ), tiles, dim3( 256 ), 0, stream, guide, buf[ src ], width, height, tiles_x, stride,
                                normal_power_log2, sigma_plane, sigma_lum, buf[ src ^ 1 ], ( const double* )nullptr, ( const double* )nullptr, 0u, ( double* )nullptr );
        else
            hipLaunchKernelGGL( ( k_dn_level< true > ), tiles, dim3( 256 ), 0, stream, guide, buf[ src ], width, height, tiles_x, stride,
                                normal_power_log2, sigma_plane, sigma_lum, ( double2* )nullptr, lin, surf, no_demodulate, out_rgb );
    }
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
    int src = 1;
    for( uint32_t i = 0; i < iterations; i++, src ^= 1 )
    {
        const long long stride = 1ll << i;
        if( i + 1 < iterations )
            hipLaunchKernelGGL( ( k_dn_level< false > ), tiles, dim3( 256 ), 0, stream, guide, buf[ src ], width, height, tiles_x, stride,
                                normal_power_log2, sigma_plane, sigma_lum, buf[ src ^ 1 ], ( const double* )nullptr, ( const double* )nullptr, 0u, ( double* )nullptr );
        else
            hipLaunchKernelGGL( ( k_dn_level< true > ), tiles, dim3( 256 ), 0, stream, guide, buf[ src ], width, height, tiles_x, stride,
                                normal_power_log2, sigma_plane, sigma_lum, ( double2* )nullptr, ( const double* )out_rgb, surf, no_demodulate, out_rgb );
    }
}
