/* k_fill.hip -- acn_fill_stats: the unrendered positions of a sparse frame from their rendered neighbours (include/actinon_hip.h
 * states every expression and its order; tests/fill_model.py restates them in numpy and the two are compared bit for bit).
 *
 * Launches of one call: k_fill_prepare, k_fill_gather.
 *   prepare  one pixel per lane: reads the lane's 64-byte statistics record and its 128-byte surface record with 16-byte loads and
 *            writes what a tap needs as aligned pieces: a 64-byte guide -- N, P and the key, whose fourth word holds the bits
 *            FILL_DONOR, FILL_PRESENT (the record is not EMPTY), FILL_VAR (n > 1) and FILL_RECEIVER -- and 48 bytes { c.xyz, u.xyz },
 *            c = mean / a, u = vm / ( a * a ).  It also writes the output of every position as if no receiver were filled: the
 *            record and -1 (RENDERED), the background and 0 (BACKGROUND), the EMPTY record and +inf (everything else).
 *   gather   the tiles of k_dn_level (acn_denoise_dev.h): 256-lane workgroups on 16 x 16 pixel tiles numbered in blockIdx.x, lane t
 *            on pixel ( t & 15, t >> 4 ).  A workgroup with no receiver lane leaves at once (every workgroup of a finished frame).
 *            Else it stages its tile and the halo of R pixels around it in LDS, ( 16 + 2 R )^2 entries in seven planes of 16-byte
 *            pieces: the key of every entry (a zero key off the image: neither rendered nor a donor), and N, P, c, u of the donors
 *            alone -- of a lattice of every second pixel three entries in four are EMPTY and cost 16 bytes.  53 KB at R = 3 (two
 *            workgroups on a CU), 112 KB at R = 8 (one).  After the one barrier a wave with no receiver lane leaves, and the
 *            ( 2 R + 1 )^2 taps are read from LDS: per tap the key, then the six pieces.  A tap that is skipped is predicated: it is
 *            read and a select drops its terms -- sums start at +0 and never become -0, so adding the +0 of a dropped term is adding
 *            nothing.  The two branches in the window are wave-level: a tap at which no lane of the wave finds a rendered record, or
 *            none a donor of its surface, is not read further, which for the same reason changes no bit.  A FILLED lane overwrites
 *            what prepare wrote for it; no lane reads another lane's registers, and a result does not depend on the tile it is in.
 * The same gather read through the cache (per tap 16 bytes of key, then 96 bytes of the tap's pixel, as the denoiser's levels do) was
 * measured beside this one and is not kept: DESIGN.md section 7, profiles/r26/NOTES.md. */
#include <hip/hip_runtime.h>
#include "acn_launch.h"
#include "acn_denoise_dev.h"

#define FILL_DONOR    1
#define FILL_PRESENT  2
#define FILL_VAR      4
#define FILL_RECEIVER 8

__global__ __launch_bounds__( 256 )
void k_fill_prepare( const double2* __restrict__ stats, const double* __restrict__ surf, size_t n, uint32_t no_demodulate,
                     double bg_x, double bg_y, double bg_z, double2* __restrict__ guide, double2* __restrict__ pix,
                     double2* __restrict__ out_stats, double* __restrict__ out_need )
{
    const size_t i = ( size_t )blockIdx.x * blockDim.x + threadIdx.x;
    if( i >= n ) return;
    const double2 s0 = stats[ 4 * i ], s1 = stats[ 4 * i + 1 ], s2 = stats[ 4 * i + 2 ], s3 = stats[ 4 * i + 3 ];
    const double2* r = ( const double2* )( surf + ( size_t )ACN_SURF_STRIDE * i );
    const double2 r0 = r[ 0 ], r1 = r[ 1 ], r2 = r[ 2 ], r3 = r[ 3 ], r4 = r[ 4 ], r5 = r[ 5 ], r6 = r[ 6 ];
    const bool empty = stats_empty( s0.x );
    const bool hit = r0.x < __builtin_inf();
    const bool emitter = ( ( uint32_t )( int32_t )r6.x & ACN_SURF_EMITTER ) != 0;
    const double ax = dn_albedo( r4.y, no_demodulate ), ay = dn_albedo( r5.x, no_demodulate ), az = dn_albedo( r5.y, no_demodulate );
    const double cx = s0.y / ax, cy = s1.x / ay, cz = s1.y / az;
    const double cnt = s0.x;
    const bool var = !empty && cnt > 1.0;
    const double ux = stats_var_of_mean( s2.x, cnt ) / ( ax * ax ), uy = stats_var_of_mean( s2.y, cnt ) / ( ay * ay ),
                 uz = stats_var_of_mean( s3.x, cnt ) / ( az * az );
    const bool donor = !empty && hit && !emitter && dn_finite( cx ) && dn_finite( cy ) && dn_finite( cz );
    const bool receiver = empty && hit && !emitter && dn_finite( r2.x ) && dn_finite( r2.y ) && dn_finite( r3.x )
                          && dn_finite( r0.y ) && dn_finite( r1.x ) && dn_finite( r1.y );
    DnKey key;
    key.enter = ( int32_t )r3.y; key.exit = ( int32_t )r4.x; key.hops = ( int32_t )r6.y;
    key.ok = ( donor ? FILL_DONOR : 0 ) | ( empty ? 0 : FILL_PRESENT ) | ( var ? FILL_VAR : 0 ) | ( receiver ? FILL_RECEIVER : 0 );
    union { DnKey k; double2 d; } kv; kv.k = key;
    double2* g = guide + 4 * i;
    g[ 0 ] = make_double2( r2.x, r2.y );   /* N */
    g[ 1 ] = make_double2( r3.x, r0.y );   /* N.z, P.x */
    g[ 2 ] = make_double2( r1.x, r1.y );   /* P.y, P.z */
    g[ 3 ] = kv.d;
    pix[ 3 * i ]     = make_double2( cx, cy );
    pix[ 3 * i + 1 ] = make_double2( cz, ux );
    pix[ 3 * i + 2 ] = make_double2( uy, uz );
    const bool background = empty && !hit;
    out_stats[ 4 * i ]     = background ? make_double2( 1.0, bg_x ) : s0;
    out_stats[ 4 * i + 1 ] = background ? make_double2( bg_y, bg_z ) : s1;
    out_stats[ 4 * i + 2 ] = background ? make_double2( 0.0, 0.0 ) : s2;
    out_stats[ 4 * i + 3 ] = background ? make_double2( 0.0, 0.0 ) : s3;
    if( out_need ) out_need[ i ] = !empty ? -1.0 : ( background ? 0.0 : __builtin_inf() );
}


/* the receiver of a gather -- N, P, its key -- and its nine sums */
struct FillCentre { double nx, ny, nz, px, py, pz; DnKey key; };
struct FillSums { double sa, sw, swv, scx, scy, scz, sux, suy, suz; };

/* the tap's record is rendered and, with `take`, a donor of the receiver's surface */
__device__ static inline bool fill_present( const DnKey& k2 ) { return ( k2.ok & FILL_PRESENT ) != 0; }
__device__ static inline bool fill_takes( const FillCentre& c, const DnKey& k2 )
{
    return ( k2.ok & FILL_DONOR ) && k2.enter == c.key.enter && k2.exit == c.key.exit && k2.hops == c.key.hops;
}

/* one donor tap: w from the receiver and the tap's guide ( h0 .. h2 ), its terms from the tap's { c, u } pieces ( t0 .. t2 ), predicated */
__device__ static inline void fill_tap_add( FillSums& s, const FillCentre& c, double ts, double2 h0, double2 h1, double2 h2, double2 t0, double2 t1, double2 t2,
                                            bool take, bool tv, uint32_t normal_power_log2, double sigma_plane )
{
    double wn = dn_dot( c.nx, c.ny, c.nz, h0.x, h0.y, h1.x );
    wn = wn > 0 ? wn : 0.0;
    for( uint32_t j = 0; j < normal_power_log2; j++ ) wn = wn * wn;
    const double ex = h1.y - c.px, ey = h2.x - c.py, ez = h2.y - c.pz;
    const double len = acn_sqrt( dn_dot( ex, ey, ez, ex, ey, ez ) );
    const double tp = len > 0 ? ( acn_fabs( dn_dot( c.nx, c.ny, c.nz, ex, ey, ez ) ) / len ) / sigma_plane : 0.0;
    const double w = wn * acn_exp( -( ts + tp ) );
    s.sw  += take ? w : 0.0;
    s.scx += take ? w * t0.x : 0.0;
    s.scy += take ? w * t0.y : 0.0;
    s.scz += take ? w * t1.x : 0.0;
    s.swv += tv ? w : 0.0;
    s.sux += tv ? w * t1.y : 0.0;
    s.suy += tv ? w * t2.x : 0.0;
    s.suz += tv ? w * t2.y : 0.0;
}

/* the record and the need of a FILLED position p; an UNFILLED one keeps what prepare wrote */
__device__ static inline void fill_write( const FillSums& s, const double* __restrict__ surf, size_t p, uint32_t no_demodulate,
                                          double2* __restrict__ out_stats, double* __restrict__ out_need )
{
    const double2* r = ( const double2* )( surf + ( size_t )ACN_SURF_STRIDE * p );
    const double2 r4 = r[ 4 ], r5 = r[ 5 ];
    const double ax = dn_albedo( r4.y, no_demodulate ), ay = dn_albedo( r5.x, no_demodulate ), az = dn_albedo( r5.y, no_demodulate );
    const bool var = s.swv > 0;
    const double m2x = var ? ( ( s.sux / s.swv ) * ( ax * ax ) ) * 2.0 : 0.0;
    const double m2y = var ? ( ( s.suy / s.swv ) * ( ay * ay ) ) * 2.0 : 0.0;
    const double m2z = var ? ( ( s.suz / s.swv ) * ( az * az ) ) * 2.0 : 0.0;
    out_stats[ 4 * p ]     = make_double2( var ? 2.0 : 1.0, ( s.scx / s.sw ) * ax );
    out_stats[ 4 * p + 1 ] = make_double2( ( s.scy / s.sw ) * ay, ( s.scz / s.sw ) * az );
    out_stats[ 4 * p + 2 ] = make_double2( m2x, m2y );
    out_stats[ 4 * p + 3 ] = make_double2( m2z, 0.0 );
    if( out_need ) out_need[ p ] = 1.0 - s.sw / s.sa;
}

__device__ static inline FillCentre fill_centre( const double2* __restrict__ guide, size_t p, const DnKey& key )
{
    const double2 g0 = guide[ 4 * p ], g1 = guide[ 4 * p + 1 ], g2 = guide[ 4 * p + 2 ];
    FillCentre c;
    c.nx = g0.x; c.ny = g0.y; c.nz = g1.x; c.px = g1.y; c.py = g2.x; c.pz = g2.y; c.key = key;
    return c;
}

/* the tile and its halo in LDS: FILL_PLANES planes of ( DN_TILE + 2 R )^2 16-byte pieces -- plane 0 the keys, 1 .. 3 N and P, 4 .. 6
 * c and u -- so that the lanes of a wave read consecutive pieces of one plane */
#define FILL_PLANES 7
extern __shared__ double2 fill_lds[];
static size_t fill_lds_bytes( uint32_t radius )
{
    const size_t S = DN_TILE + 2 * ( size_t )radius;
    return FILL_PLANES * S * S * sizeof( double2 );
}
static_assert( FILL_PLANES * ( DN_TILE + 2 * ACN_FILL_MAX_RADIUS ) * ( DN_TILE + 2 * ACN_FILL_MAX_RADIUS ) * 16 <= 160 * 1024, "the largest halo fits the LDS of a CU" );

__global__ __launch_bounds__( 256 )
void k_fill_gather( const double2* __restrict__ guide, const double2* __restrict__ pix, const double* __restrict__ surf, size_t width, size_t height,
                    size_t tiles_x, int radius, uint32_t normal_power_log2, uint32_t no_demodulate, double sigma_px, double sigma_plane,
                    double2* __restrict__ out_stats, double* __restrict__ out_need )
{
    const int S = DN_TILE + 2 * radius, E = S * S;
    const size_t tile = blockIdx.x;
    const size_t ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int lx = threadIdx.x & ( DN_TILE - 1 ), ly = threadIdx.x / DN_TILE;
    const size_t x = tx * DN_TILE + lx, y = ty * DN_TILE + ly;
    const bool in_image = x < width && y < height;
    const size_t p = in_image ? y * width + x : 0;
    const DnKey key = dn_key( guide, p );   /* (a lane off the image reads pixel 0 and is no receiver) */
    const bool receiver = in_image && ( key.ok & FILL_RECEIVER );
    if( !__syncthreads_or( receiver ) ) return;   /* workgroup-level: nothing to fill in this tile */
    const long long x0 = ( long long )( tx * DN_TILE ) - radius, y0 = ( long long )( ty * DN_TILE ) - radius;
    for( int e = threadIdx.x; e < E; e += 256 )
    {
        const int ey = e / S, ex = e - ey * S;
        const long long qx = x0 + ex, qy = y0 + ey;
        const bool inside = qx >= 0 && qx < ( long long )width && qy >= 0 && qy < ( long long )height;
        double2 kd = make_double2( 0.0, 0.0 );   /* ok = 0: neither rendered nor a donor */
        if( inside )
        {
            const size_t q = ( size_t )qy * width + ( size_t )qx;
            kd = guide[ 4 * q + 3 ];
            union { DnKey k; double2 d; } kv; kv.d = kd;
            if( kv.k.ok & FILL_DONOR )   /* (no tap is taken from another entry: its planes stay as they are and are dropped by the selects) */
            {
                fill_lds[ 1 * E + e ] = guide[ 4 * q ]; fill_lds[ 2 * E + e ] = guide[ 4 * q + 1 ]; fill_lds[ 3 * E + e ] = guide[ 4 * q + 2 ];
                fill_lds[ 4 * E + e ] = pix[ 3 * q ];   fill_lds[ 5 * E + e ] = pix[ 3 * q + 1 ];   fill_lds[ 6 * E + e ] = pix[ 3 * q + 2 ];
            }
        }
        fill_lds[ e ] = kd;
    }
    __syncthreads();
    if( !__any( receiver ) ) return;   /* wave-level: nothing to fill here; no barrier follows */
    const FillCentre c = fill_centre( guide, p, key );
    const double s2 = sigma_px * sigma_px;
    FillSums s = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
    #pragma unroll 1
    for( int dy = -radius; dy <= radius; dy++ )
    {
        #pragma unroll 1
        for( int dx = -radius; dx <= radius; dx++ )
        {
            const int e = ( ly + radius + dy ) * S + ( lx + radius + dx );
            union { DnKey k; double2 d; } kv; kv.d = fill_lds[ e ];
            const DnKey k2 = kv.k;
            const bool present = receiver && fill_present( k2 );
            if( !__any( present ) ) continue;   /* wave-level: no lane has a rendered record at this tap */
            const double ts = ( double )( dx * dx + dy * dy ) / s2;
            s.sa += present ? acn_exp( -ts ) : 0.0;
            const bool take = present && fill_takes( c, k2 );
            if( !__any( take ) ) continue;      /* wave-level: no lane takes this tap */
            fill_tap_add( s, c, ts, fill_lds[ 1 * E + e ], fill_lds[ 2 * E + e ], fill_lds[ 3 * E + e ], fill_lds[ 4 * E + e ], fill_lds[ 5 * E + e ],
                          fill_lds[ 6 * E + e ], take, take && ( k2.ok & FILL_VAR ), normal_power_log2, sigma_plane );
        }
    }
    if( receiver && s.sw > 0 ) fill_write( s, surf, p, no_demodulate, out_stats, out_need );
}

/* scratch: [ n ] guides of 64 bytes, then [ n ] pieces of 48 bytes (ACN_FILL_SCRATCH_PER_PIXEL in all) */
void acn_launch_fill_stats( const double* stats, const double* surf, size_t width, size_t height, uint32_t radius, uint32_t normal_power_log2,
                            uint32_t no_demodulate, double sigma_px, double sigma_plane, const double* background, void* scratch,
                            double* out_stats, double* out_need, hipStream_t stream )
{
    const size_t n = width * height;
    double2* guide = ( double2* )scratch;
    double2* pix = guide + 4 * n;
    const size_t tiles_x = ( width + DN_TILE - 1 ) / DN_TILE, tiles_y = ( height + DN_TILE - 1 ) / DN_TILE;
    const dim3 tiles( ( unsigned )( tiles_x * tiles_y ) );   /* n <= 2^31: at most 2^27 + 2^23 tiles */
    hipLaunchKernelGGL( k_fill_prepare, dim3( ( unsigned )( ( n + 255 ) / 256 ) ), dim3( 256 ), 0, stream, ( const double2* )stats, surf, n, no_demodulate,
                        background[ 0 ], background[ 1 ], background[ 2 ], guide, pix, ( double2* )out_stats, out_need );
    /* from R = 5 on a launch asks for more than the 64 KB it may have by default.  The bound is raised to the largest halo's on the
     * call's device every time, never to this call's own: two threads with different radii then cannot undercut each other.  (Refused:
     * so is the launch, and the caller reads hipGetLastError.) */
    ( void )hipFuncSetAttribute( ( const void* )k_fill_gather, hipFuncAttributeMaxDynamicSharedMemorySize, ( int )fill_lds_bytes( ACN_FILL_MAX_RADIUS ) );
    const size_t lds = fill_lds_bytes( radius );
    hipLaunchKernelGGL( k_fill_gather, tiles, dim3( 256 ), lds, stream, guide, pix, surf, width, height, tiles_x, ( int )radius, normal_power_log2,
                        no_demodulate, sigma_px, sigma_plane, ( double2* )out_stats, out_need );
}
