/* acn_denoise_dev.h -- what the kernels of the edge-avoiding filter share (k_denoise.hip, k_denoise_layers.hip): the small
 * expressions of include/actinon_hip.h (lum, dot, the a-trous kernel, the albedo rule), the arrangement of the window kernels
 * (256-lane workgroups on 16 x 16 pixel tiles, numbered in blockIdx.x) and one body per step -- the guide of an entry and its match
 * key (dn_guide, dn_match), var_raw (dn_var_raw), the 3 x 3 prefilter (dn_prefilter) and the a-trous level (dn_tap_add, dn_level).
 * An ENTRY is what a lane filters: pixel p of the plain filter, ( layer, pixel ) = l * n + p of the layered one.  The two window
 * bodies are templates over a tap SOURCE, which names the entry a tap is read from and whether it counts: DnPixelSource here, the
 * candidate rule of k_denoise_layers.hip there.  Everything is inlined; a kernel keeps what is its own. */
#ifndef ACN_DENOISE_DEV_H
#define ACN_DENOISE_DEV_H

#include <hip/hip_runtime.h>
#include "acn_launch.h"
#include "acn_stats_dev.h"

#define DN_TILE 16

struct DnKey { int32_t enter, exit, hops, ok; };   /* ok: the pixel is filterable */

__device__ static inline bool dn_finite( double x ) { return ( acn_f64_bits( x ) & 0x7FF0000000000000ull ) != 0x7FF0000000000000ull; }
__device__ static inline double dn_lum( double x, double y, double z ) { return ( 0.2126 * x + 0.7152 * y ) + 0.0722 * z; }
__device__ static inline double dn_dot( double ax, double ay, double az, double bx, double by, double bz ) { return ( ax * bx + ay * by ) + az * bz; }
__device__ static inline double dn_k( int t ) { return t == 2 ? 0.375 : ( ( t & 1 ) ? 0.25 : 0.0625 ); }
__device__ static inline double dn_albedo( double v, uint32_t no_demodulate ) { return ( !no_demodulate && v > 0.01 ) ? v : 1.0; }

/* the pixel of this lane; false: outside the image */
__device__ static inline bool dn_pixel( size_t width, size_t height, size_t tiles_x, size_t* x, size_t* y )
{
    const size_t tile = blockIdx.x;
    const size_t ty = tile / tiles_x, tx = tile - ty * tiles_x;
    *x = tx * DN_TILE + ( threadIdx.x & ( DN_TILE - 1 ) );
    *y = ty * DN_TILE + ( threadIdx.x / DN_TILE );
    return *x < width && *y < height;
}

__device__ static inline DnKey dn_key( const double2* __restrict__ guide, size_t p )
{
    union { DnKey k; double2 d; } kv; kv.d = guide[ 4 * p + 3 ];
    return kv.k;
}

/* k2 is filterable and of the class of `key` */
__device__ static inline bool dn_match( DnKey key, DnKey k2 )
{
    return k2.ok && k2.enter == key.enter && k2.exit == key.exit && k2.hops == key.hops;
}

/* var_raw of a statistics record ( s0, s2, s3: its pieces but the second ) over the albedo divisors: the measured variance of the
 * demodulated mean's luminance, -1 for none */
__device__ static inline double dn_var_raw( double2 s0, double2 s2, double2 s3, double ax, double ay, double az )
{
    const double cnt = s0.x;
    if( stats_empty( cnt ) || !( cnt > 1.0 ) ) return -1.0;
    const double vx = stats_var_of_mean( s2.x, cnt ), vy = stats_var_of_mean( s2.y, cnt ), vz = stats_var_of_mean( s3.x, cnt );
    return ( ( 0.2126 * 0.2126 ) * ( vx / ( ax * ax ) ) + ( 0.7152 * 0.7152 ) * ( vy / ( ay * ay ) ) ) + ( 0.0722 * 0.0722 ) * ( vz / ( az * az ) );
}

/* What a tap needs of entry i, as two aligned pieces: the 64-byte guide -- N, P and the match key, from the entry's 128-byte surface
 * record, read with 16-byte loads (the line k_surface wrote whole) -- and 32 bytes { c.xyz, var }, c the colour ( lx, ly, lz ) over
 * the albedo divisors.  usable: what else `ok` needs (the entry has samples); STATS: var is the var_raw of the entry's statistics
 * record ( s0, s2, s3 ), else 0 */
template< bool STATS >
__device__ static inline void dn_guide( const double* __restrict__ surf, size_t i, uint32_t no_demodulate, bool usable, double lx, double ly, double lz,
                                        double2 s0, double2 s2, double2 s3, double2* __restrict__ guide, double2* __restrict__ pix )
{
    const double2* r = ( const double2* )( surf + ( size_t )ACN_SURF_STRIDE * i );
    const double2 r0 = r[ 0 ], r1 = r[ 1 ], r2 = r[ 2 ], r3 = r[ 3 ], r4 = r[ 4 ], r5 = r[ 5 ], r6 = r[ 6 ];
    const double ax = dn_albedo( r4.y, no_demodulate ), ay = dn_albedo( r5.x, no_demodulate ), az = dn_albedo( r5.y, no_demodulate );
    const double cx = lx / ax, cy = ly / ay, cz = lz / az;
    DnKey key;
    key.enter = ( int32_t )r3.y; key.exit = ( int32_t )r4.x; key.hops = ( int32_t )r6.y;
    key.ok = usable && r0.x < __builtin_inf() && !( ( uint32_t )( int32_t )r6.x & ACN_SURF_EMITTER ) && dn_finite( cx ) && dn_finite( cy ) && dn_finite( cz );
    double var = 0.0;
    if constexpr( STATS ) var = dn_var_raw( s0, s2, s3, ax, ay, az );
    union { DnKey k; double2 d; } kv; kv.k = key;
    double2* g = guide + 4 * i;
    g[ 0 ] = make_double2( r2.x, r2.y );   /* N */
    g[ 1 ] = make_double2( r3.x, r0.y );   /* N.z, P.x */
    g[ 2 ] = make_double2( r1.x, r1.y );   /* P.y, P.z */
    g[ 3 ] = kv.d;
    pix[ 2 * i ]     = make_double2( cx, cy );
    pix[ 2 * i + 1 ] = make_double2( cz, var );
}

/* the in-image pixel ( x + dx, y + dy ), or the centre p with *in = false */
__device__ static inline size_t dn_tap( size_t x, size_t y, long long dx, long long dy, size_t width, size_t height, size_t p, bool* in )
{
    const long long qx = ( long long )x + dx, qy = ( long long )y + dy;
    *in = qx >= 0 && qx < ( long long )width && qy >= 0 && qy < ( long long )height;
    return *in ? ( size_t )qy * width + ( size_t )qx : p;
}

/* The tap source of the plain filter: tap pixel q itself, taken if it is in the image and matches.  A SOURCE answers
 * entry( guide, q, inside, centre, key, &ok ): the entry the tap at pixel q is read from -- in the image, or q == p with inside
 * false; centre: the tap is the centre itself -- and whether the tap counts; a tap that does not count still names a readable entry */
struct DnPixelSource
{
    __device__ size_t entry( const double2* __restrict__ guide, size_t q, bool inside, bool centre, const DnKey& key, bool* ok ) const
    {
        const bool match = dn_match( key, dn_key( guide, q ) );   /* (whatever `inside` says: a tap off the image is predicated) */
        *ok = inside && match;
        return q;
    }
};

/* var of the lane's entry (pixel ( x, y ) = p, key `key`, in = { c.xyz, var_raw }): the ( 1/4, 1/2, 1/4 )^2 mean of the var_raw that
 * the taps of the 3 x 3 window which count have; 0 where none has one or the entry is not filterable */
template< class SOURCE >
__device__ static inline double dn_prefilter( const SOURCE& src, const double2* __restrict__ guide, const double2* __restrict__ in,
                                              size_t x, size_t y, size_t p, const DnKey& key, size_t width, size_t height )
{
    if( !key.ok ) return 0.0;
    double sw = 0.0, sv = 0.0;
    #pragma unroll
    for( int dy = -1; dy <= 1; dy++ )
    {
        #pragma unroll
        for( int dx = -1; dx <= 1; dx++ )
        {
            bool inside, found;
            const size_t q = dn_tap( x, y, dx, dy, width, height, p, &inside );
            const size_t e = src.entry( guide, q, inside, dx == 0 && dy == 0, key, &found );
            const double vr = in[ 2 * e + 1 ].y;
            const bool ok = found && !( vr < 0.0 );
            const double g = ( dy ? 0.25 : 0.5 ) * ( dx ? 0.25 : 0.5 );
            sw += ok ? g : 0.0;
            sv += ok ? g * vr : 0.0;
        }
    }
    return sw > 0 ? sv / sw : 0.0;
}

/* the centre of a level -- N, P, the colour pieces, l and den -- and its five sums */
struct DnCentre { double nx, ny, nz, px, py, pz, l, den; double2 c0, c1; };
struct DnSums { double sw, sx, sy, sz, sv; };

/* one tap of a level: w from the centre and the tap's guide ( h0 .. h2 ) and colour ( t0, t1 ) pieces, kk = dn_k( tj ) * dn_k( ti ),
 * and its five terms, predicated: sums start at +0 and never become -0, so adding the +0 of a dropped term is adding nothing */
__device__ static inline void dn_tap_add( DnSums& s, const DnCentre& c, double2 h0, double2 h1, double2 h2, double2 t0, double2 t1, double kk,
                                          bool centre, bool ok, uint32_t normal_power_log2, double sigma_plane )
{
    double wn = dn_dot( c.nx, c.ny, c.nz, h0.x, h0.y, h1.x );
    wn = wn > 0 ? wn : 0.0;
    for( uint32_t k = 0; k < normal_power_log2; k++ ) wn = wn * wn;
    const double dx = h1.y - c.px, dy = h2.x - c.py, dz = h2.y - c.pz;
    const double len = acn_sqrt( dn_dot( dx, dy, dz, dx, dy, dz ) );
    const double tp = len > 0 ? ( acn_fabs( dn_dot( c.nx, c.ny, c.nz, dx, dy, dz ) ) / len ) / sigma_plane : 0.0;
    const double tl = acn_fabs( dn_lum( t0.x, t0.y, t1.x ) - c.l ) / c.den;
    double w = ( kk * wn ) * acn_exp( -( tp + tl ) );
    if( centre ) w = 0.375 * 0.375;
    s.sw += ok ? w : 0.0;
    s.sx += ok ? w * ( t0.x - c.c0.x ) : 0.0;
    s.sy += ok ? w * ( t0.y - c.c0.y ) : 0.0;
    s.sz += ok ? w * ( t1.x - c.c1.x ) : 0.0;
    s.sv += ok ? ( w * w ) * t1.y : 0.0;
}

/* one a-trous level for the filterable entry `self` (pixel ( x, y ) = p, key `key`): 5 x 5 taps at `stride`, a gather: per tap the
 * source's keys, then 48 bytes of N, P and 32 bytes of colour.  The one branch is wave-level: a tap that no lane of the wave takes
 * (most of them at stride 64 near a border) is not loaded, which changes no bit.  Returns { c.x, c.y } and { c.z, var } of the output */
template< class SOURCE >
__device__ static inline void dn_level( const SOURCE& src, const double2* __restrict__ guide, const double2* __restrict__ in, size_t x, size_t y,
                                        size_t p, size_t self, const DnKey& key, size_t width, size_t height, long long stride,
                                        uint32_t normal_power_log2, double sigma_plane, double sigma_lum, double2* o0, double2* o1 )
{
    const double2 g0 = guide[ 4 * self ], g1 = guide[ 4 * self + 1 ], g2 = guide[ 4 * self + 2 ];
    DnCentre c;
    c.nx = g0.x; c.ny = g0.y; c.nz = g1.x; c.px = g1.y; c.py = g2.x; c.pz = g2.y;
    c.c0 = in[ 2 * self ]; c.c1 = in[ 2 * self + 1 ];
    c.l = dn_lum( c.c0.x, c.c0.y, c.c1.x );
    c.den = sigma_lum * acn_sqrt( c.c1.y ) + 1e-8;
    DnSums s = { 0.0, 0.0, 0.0, 0.0, 0.0 };
    #pragma unroll 1
    for( int tj = 0; tj < 5; tj++ )
    {
        #pragma unroll
        for( int ti = 0; ti < 5; ti++ )
        {
            const bool centre = tj == 2 && ti == 2;
            bool inside, ok;
            const size_t q = dn_tap( x, y, ( ti - 2 ) * stride, ( tj - 2 ) * stride, width, height, p, &inside );
            const size_t e = src.entry( guide, q, inside, centre, key, &ok );
            if( !__any( ok ) ) continue;   /* wave-level: no lane takes this tap */
            dn_tap_add( s, c, guide[ 4 * e ], guide[ 4 * e + 1 ], guide[ 4 * e + 2 ], in[ 2 * e ], in[ 2 * e + 1 ], dn_k( tj ) * dn_k( ti ),
                        centre, ok, normal_power_log2, sigma_plane );
        }
    }
    *o0 = make_double2( c.c0.x + s.sx / s.sw, c.c0.y + s.sy / s.sw );
    *o1 = make_double2( c.c1.x + s.sz / s.sw, s.sv / ( s.sw * s.sw ) );
}

#endif
