/* k_denoise_layers.hip -- the layered filter of acn_denoise_layers (include/actinon_hip.h states the candidate rule and the composite;
 * steps 1 to 4 are those of acn_denoise_stats; tests/lens_layers_model.py restates all of it in numpy, compared bit for bit).
 *
 * A pixel has two layers, each with its own statistics and surface record, and a rest.  The buffers are planar, [ layer ][ pixel ],
 * so entry l * n + p of a buffer is layer l of pixel p and the per-record kernels see 2 n records.
 * Launches of one call: k_dnl_prepare, k_dnl_prefilter, k_dnl_level once per level, k_dnl_composite.
 *   prepare    one ( pixel, layer ) per lane: k_dn_prepare_stats without the frame -- the 64-byte guide and { c.xyz, var_raw }.
 *   prefilter  the 3 x 3 window of k_dn_prefilter; level: the 5 x 5 taps of k_dn_level.  Both run the tiles of k_denoise.hip with the
 *              layer in blockIdx.y, so a wave holds pixels of one layer.  Per tap the keys of both layers of the tap pixel are
 *              loaded (2 x 16 bytes) and the CANDIDATE is chosen -- the centre's own layer at the centre, else the lowest layer
 *              that is filterable and matches -- then N, P and the colour come from the candidate's entries.  A tap without a
 *              candidate is predicated as in k_dn_level: its address is the centre's entry, a select drops its terms.
 *   composite  one pixel per lane: F_l = c * a of the last level's output, or the mean of a layer that is not filterable; the terms
 *              ( n_l / K_p ) * F_l and the rest's, added in the order layer 0, layer 1, rest from the first term present.
 * The levels ping-pong both layers between two colour buffers [ 2 ][ n ]; no lane reads another lane's registers.
 * Scratch: [ 2 n ] guides of 64 bytes, two colour buffers [ 2 n ] of 32 bytes: 256 bytes per pixel. */
#include <hip/hip_runtime.h>
#include "acn_launch.h"
#include "acn_denoise_dev.h"

/* a record whose [ 0 ] is not a finite number >= 1 is EMPTY */
__device__ static inline bool dnl_empty( double n ) { return !( n >= 1.0 && n < __builtin_inf() ); }

/* steps 1 and 2 of acn_denoise_stats for entry i of the 2 n ( layer, pixel ) entries */
__global__ __launch_bounds__( 256 )
void k_dnl_prepare( const double2* __restrict__ stats, const double* __restrict__ surf, size_t entries, uint32_t no_demodulate,
                    double2* __restrict__ guide, double2* __restrict__ pix )
{
    const size_t i = ( size_t )blockIdx.x * blockDim.x + threadIdx.x;
    if( i >= entries ) return;
    const double2 s0 = stats[ 4 * i ], s1 = stats[ 4 * i + 1 ], s2 = stats[ 4 * i + 2 ], s3 = stats[ 4 * i + 3 ];
    const double2* r = ( const double2* )( surf + ( size_t )ACN_SURF_STRIDE * i );
    const double2 r0 = r[ 0 ], r1 = r[ 1 ], r2 = r[ 2 ], r3 = r[ 3 ], r4 = r[ 4 ], r5 = r[ 5 ], r6 = r[ 6 ];
    const double cnt = s0.x;
    const bool empty = dnl_empty( cnt );
    const double ax = dn_albedo( r4.y, no_demodulate ), ay = dn_albedo( r5.x, no_demodulate ), az = dn_albedo( r5.y, no_demodulate );
    const double cx = s0.y / ax, cy = s1.x / ay, cz = s1.y / az;
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
}

/* The candidate of tap pixel q for the centre entry `self` (a filterable layer of pixel p, key `key`): the entry it is read from, or
 * `self` with *ok = false.  centre: the tap is the centre itself; inside: q is in the image (else q == p and nothing is taken) */
__device__ static inline size_t dnl_candidate( const double2* __restrict__ guide, size_t n, size_t q, size_t self, const DnKey& key, bool centre,
                                               bool inside, bool* ok )
{
    if( centre ) { *ok = true; return self; }
    const DnKey k0 = dn_key( guide, q ), k1 = dn_key( guide, n + q );
    const bool m0 = inside && k0.ok && k0.enter == key.enter && k0.exit == key.exit && k0.hops == key.hops;
    const bool m1 = inside && k1.ok && k1.enter == key.enter && k1.exit == key.exit && k1.hops == key.hops;
    *ok = m0 || m1;
    return m0 ? q : m1 ? n + q : self;
}

/* k_dn_prefilter over the candidates; blockIdx.y: the layer */
__global__ __launch_bounds__( 256 )
void k_dnl_prefilter( const double2* __restrict__ guide, const double2* __restrict__ in, size_t width, size_t height, size_t tiles_x,
                      double2* __restrict__ out )
{
    size_t x, y;
    if( !dn_pixel( width, height, tiles_x, &x, &y ) ) return;
    const size_t n = width * height, p = y * width + x, self = ( size_t )blockIdx.y * n + p;
    const DnKey key = dn_key( guide, self );
    const double2 c0 = in[ 2 * self ], c1 = in[ 2 * self + 1 ];
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
                bool inside, found;
                const size_t q = dn_tap( x, y, dx, dy, width, height, p, &inside );
                const size_t e = dnl_candidate( guide, n, q, self, key, dx == 0 && dy == 0, inside, &found );
                const double vr = in[ 2 * e + 1 ].y;
                const bool ok = found && !( vr < 0.0 );
                const double g = ( dy ? 0.25 : 0.5 ) * ( dx ? 0.25 : 0.5 );
                sw += ok ? g : 0.0;
                sv += ok ? g * vr : 0.0;
            }
        }
        var = sw > 0 ? sv / sw : 0.0;
    }
    out[ 2 * self ]     = c0;
    out[ 2 * self + 1 ] = make_double2( c1.x, var );
}

/* one a-trous level of k_dn_level over the candidates; blockIdx.y: the layer.  An entry that is not filterable is left alone */
__global__ __launch_bounds__( 256 )
void k_dnl_level( const double2* __restrict__ guide, const double2* __restrict__ in, size_t width, size_t height, size_t tiles_x,
                  long long stride, uint32_t normal_power_log2, double sigma_plane, double sigma_lum, double2* __restrict__ out )
{
    size_t x, y;
    if( !dn_pixel( width, height, tiles_x, &x, &y ) ) return;
    const size_t n = width * height, p = y * width + x, self = ( size_t )blockIdx.y * n + p;
    const DnKey key = dn_key( guide, self );
    if( !key.ok ) return;
    const double2 g0 = guide[ 4 * self ], g1 = guide[ 4 * self + 1 ], g2 = guide[ 4 * self + 2 ];
    const double nx = g0.x, ny = g0.y, nz = g1.x, px = g1.y, py = g2.x, pz = g2.y;
    const double2 c0 = in[ 2 * self ], c1 = in[ 2 * self + 1 ];
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
            bool inside, ok;
            const size_t q = dn_tap( x, y, ( ti - 2 ) * stride, ( tj - 2 ) * stride, width, height, p, &inside );
            const size_t e = dnl_candidate( guide, n, q, self, key, centre, inside, &ok );
            if( !__any( ok ) ) continue;   /* wave-level: no lane takes this tap */
            const double2 h0 = guide[ 4 * e ], h1 = guide[ 4 * e + 1 ], h2 = guide[ 4 * e + 2 ];
            const double2 t0 = in[ 2 * e ], t1 = in[ 2 * e + 1 ];
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
    out[ 2 * self ]     = make_double2( c0.x + sx / sw, c0.y + sy / sw );
    out[ 2 * self + 1 ] = make_double2( c1.x + sz / sw, sv / ( sw * sw ) );
}

/* step 4 and the composite.  fin: the output of the last level */
__global__ __launch_bounds__( 256 )
void k_dnl_composite( const double2* __restrict__ stats, const double* __restrict__ surf, const double2* __restrict__ guide,
                      const double2* __restrict__ fin, size_t n, uint32_t no_demodulate, double bg_x, double bg_y, double bg_z,
                      double* __restrict__ out_rgb )
{
    const size_t p = ( size_t )blockIdx.x * blockDim.x + threadIdx.x;
    if( p >= n ) return;
    double cnt[ 3 ], fx[ 3 ], fy[ 3 ], fz[ 3 ];
    bool empty[ 3 ];
    #pragma unroll
    for( int l = 0; l < 3; l++ )
    {
        const size_t e = ( size_t )l * n + p;
        const double2 s0 = stats[ 4 * e ], s1 = stats[ 4 * e + 1 ];
        empty[ l ] = dnl_empty( s0.x );
        cnt[ l ] = empty[ l ] ? 0.0 : s0.x;
        fx[ l ] = s0.y; fy[ l ] = s1.x; fz[ l ] = s1.y;   /* the mean: the rest, and a layer that is not filterable */
        if( l < 2 && dn_key( guide, e ).ok )
        {
            const double2* r = ( const double2* )( surf + ( size_t )ACN_SURF_STRIDE * e );
            const double2 r4 = r[ 4 ], r5 = r[ 5 ];
            const double2 c0 = fin[ 2 * e ], c1 = fin[ 2 * e + 1 ];
            fx[ l ] = c0.x * dn_albedo( r4.y, no_demodulate );
            fy[ l ] = c0.y * dn_albedo( r5.x, no_demodulate );
            fz[ l ] = c1.x * dn_albedo( r5.y, no_demodulate );
        }
    }
    const double kp = ( cnt[ 0 ] + cnt[ 1 ] ) + cnt[ 2 ];
    double ox = bg_x, oy = bg_y, oz = bg_z;
    bool have = false;
    #pragma unroll
    for( int l = 0; l < 3; l++ )
    {
        if( empty[ l ] ) continue;
        const double share = cnt[ l ] / kp;
        const double tx = share * fx[ l ], ty = share * fy[ l ], tz = share * fz[ l ];
        ox = have ? ox + tx : tx; oy = have ? oy + ty : ty; oz = have ? oz + tz : tz;
        have = true;
    }
    out_rgb[ 3 * p ] = ox; out_rgb[ 3 * p + 1 ] = oy; out_rgb[ 3 * p + 2 ] = oz;
}

/* scratch: ACN_DENOISE_LAYERS_SCRATCH_PER_PIXEL bytes per pixel.  stats [ 3 ][ n ][ 8 ], surf [ 2 ][ n ][ 16 ], both 16-byte aligned */
void acn_launch_denoise_layers( const double* stats, const double* surf, size_t width, size_t height, uint32_t iterations, uint32_t normal_power_log2,
                                uint32_t no_demodulate, double sigma_plane, double sigma_lum, const double* background, void* scratch,
                                double* out_rgb, hipStream_t stream )
{
    const size_t n = width * height;
    double2* guide = ( double2* )scratch;
    double2* buf[ 2 ] = { guide + 8 * n, guide + 12 * n };
    const size_t tiles_x = ( width + DN_TILE - 1 ) / DN_TILE, tiles_y = ( height + DN_TILE - 1 ) / DN_TILE;
    const dim3 tiles( ( unsigned )( tiles_x * tiles_y ), 2 );
    hipLaunchKernelGGL( k_dnl_prepare, dim3( ( unsigned )( ( 2 * n + 255 ) / 256 ) ), dim3( 256 ), 0, stream, ( const double2* )stats, surf, 2 * n,
                        no_demodulate, guide, buf[ 0 ] );
    hipLaunchKernelGGL( k_dnl_prefilter, tiles, dim3( 256 ), 0, stream, guide, buf[ 0 ], width, height, tiles_x, buf[ 1 ] );
    int src = 1;
    for( uint32_t i = 0; i < iterations; i++, src ^= 1 )
        hipLaunchKernelGGL( k_dnl_level, tiles, dim3( 256 ), 0, stream, guide, buf[ src ], width, height, tiles_x, 1ll << i,
                            normal_power_log2, sigma_plane, sigma_lum, buf[ src ^ 1 ] );
    hipLaunchKernelGGL( k_dnl_composite, dim3( ( unsigned )( ( n + 255 ) / 256 ) ), dim3( 256 ), 0, stream, ( const double2* )stats, surf, guide,
                        buf[ src ], n, no_demodulate, background[ 0 ], background[ 1 ], background[ 2 ], out_rgb );
}
