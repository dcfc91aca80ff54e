/* k_denoise_layers.hip -- the layered filter of acn_denoise_layers (include/actinon_hip.h states the candidate rule and the composite;
 * steps 1 to 4 are those of acn_denoise_stats; tests/lens_layers_model.py restates all of it in numpy, compared bit for bit).
 *
 * A pixel has two layers, each with its own statistics and surface record, and a rest.  The buffers are planar, [ layer ][ pixel ],
 * so entry l * n + p of a buffer is layer l of pixel p and the per-record kernels see 2 n records.
 * Launches of one call: k_dnl_prepare, k_dnl_prefilter, k_dnl_level once per level, k_dnl_composite.
 *   prepare    one ( pixel, layer ) per lane: the dn_guide of k_dn_prepare_stats, without the frame -- the 64-byte guide and
 *              { c.xyz, var_raw }.
 *   prefilter  dn_prefilter, the 3 x 3 window of k_dn_prefilter; level: dn_level, the 5 x 5 taps of k_dn_level (acn_denoise_dev.h has
 *              the one body of each).  Both run the tiles of k_denoise.hip with the layer in blockIdx.y, so a wave holds pixels of
 *              one layer, and take their taps from DnlSource: per tap the keys of both layers of the tap pixel are loaded (2 x 16
 *              bytes) and the CANDIDATE is chosen -- the centre's own layer at the centre, else the lowest layer that is filterable
 *              and matches -- then N, P and the colour come from the candidate's entries.  A tap without a candidate is predicated
 *              as in k_dn_level: its address is the centre's entry, a select drops its terms.
 *   composite  one pixel per lane: F_l = c * a of the last level's output, or the mean of a layer that is not filterable; the terms
 *              ( n_l / K_p ) * F_l and the rest's, added in the order layer 0, layer 1, rest from the first term present.
 * The levels ping-pong both layers between two colour buffers [ 2 ][ n ]; no lane reads another lane's registers.
 * Scratch: [ 2 n ] guides of 64 bytes, two colour buffers [ 2 n ] of 32 bytes: 256 bytes per pixel. */
#include <hip/hip_runtime.h>
#include "acn_launch.h"
#include "acn_denoise_dev.h"

/* steps 1 and 2 of acn_denoise_stats for entry i of the 2 n ( layer, pixel ) entries */
__global__ __launch_bounds__( 256 )
void k_dnl_prepare( const double2* __restrict__ stats, const double* __restrict__ surf, size_t entries, uint32_t no_demodulate,
                    double2* __restrict__ guide, double2* __restrict__ pix )
{
    const size_t i = ( size_t )blockIdx.x * blockDim.x + threadIdx.x;
    if( i >= entries ) return;
    const double2 s0 = stats[ 4 * i ], s1 = stats[ 4 * i + 1 ], s2 = stats[ 4 * i + 2 ], s3 = stats[ 4 * i + 3 ];
    dn_guide< true >( surf, i, no_demodulate, !stats_empty( s0.x ), s0.y, s1.x, s1.y, s0, s2, s3, guide, pix );
}

/* The tap source of the layered filter: the CANDIDATE of tap pixel q for the centre entry `self` (a filterable layer of pixel p, key
 * `key`), or `self` with *ok = false.  centre: the tap is the centre itself; inside: q is in the image (else q == p and nothing is taken) */
struct DnlSource
{
    size_t n, self;
    __device__ size_t entry( const double2* __restrict__ guide, size_t q, bool inside, bool centre, const DnKey& key, bool* ok ) const
    {
        if( centre ) { *ok = true; return self; }
        const bool k0 = dn_match( key, dn_key( guide, q ) ), k1 = dn_match( key, dn_key( guide, n + q ) );   /* (whatever `inside` says) */
        const bool m0 = inside && k0, m1 = inside && k1;
        *ok = m0 || m1;
        return m0 ? q : m1 ? n + q : self;
    }
};

/* dn_prefilter over the candidates; blockIdx.y: the layer */
__global__ __launch_bounds__( 256 )
void k_dnl_prefilter( const double2* __restrict__ guide, const double2* __restrict__ in, size_t width, size_t height, size_t tiles_x,
                      double2* __restrict__ out )
{
    size_t x, y;
    if( !dn_pixel( width, height, tiles_x, &x, &y ) ) return;
    const size_t n = width * height, p = y * width + x, self = ( size_t )blockIdx.y * n + p;
    const double2 c0 = in[ 2 * self ], c1 = in[ 2 * self + 1 ];
    const double var = dn_prefilter( DnlSource{ n, self }, guide, in, x, y, p, dn_key( guide, self ), width, height );
    out[ 2 * self ]     = c0;
    out[ 2 * self + 1 ] = make_double2( c1.x, var );
}

/* dn_level over the candidates; blockIdx.y: the layer.  An entry that is not filterable is left alone */
__global__ __launch_bounds__( 256 )
void k_dnl_level( const double2* __restrict__ guide, const double2* __restrict__ in, size_t width, size_t height, size_t tiles_x,
                  long long stride, uint32_t normal_power_log2, double sigma_plane, double sigma_lum, double2* __restrict__ out )
{
    size_t x, y;
    if( !dn_pixel( width, height, tiles_x, &x, &y ) ) return;
    const size_t n = width * height, p = y * width + x, self = ( size_t )blockIdx.y * n + p;
    const DnKey key = dn_key( guide, self );
    if( !key.ok ) return;
    double2 o0, o1;
    dn_level( DnlSource{ n, self }, guide, in, x, y, p, self, key, width, height, stride, normal_power_log2, sigma_plane, sigma_lum, &o0, &o1 );
    out[ 2 * self ] = o0; out[ 2 * self + 1 ] = o1;
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
        empty[ l ] = stats_empty( s0.x );
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
