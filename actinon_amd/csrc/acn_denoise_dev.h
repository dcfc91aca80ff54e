/* acn_denoise_dev.h -- what the kernels of the edge-avoiding filter share (k_denoise.hip, k_denoise_layers.hip): the match key of a
 * pixel's guide, the small expressions of include/actinon_hip.h (lum, dot, the a-trous kernel, the albedo rule) and the arrangement
 * of the window kernels (256-lane workgroups on 16 x 16 pixel tiles, numbered in blockIdx.x). */
#ifndef ACN_DENOISE_DEV_H
#define ACN_DENOISE_DEV_H

#include <hip/hip_runtime.h>
#include "acn_launch.h"

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

/* the in-image pixel ( x + dx, y + dy ), or the centre p with *in = false */
__device__ static inline size_t dn_tap( size_t x, size_t y, long long dx, long long dy, size_t width, size_t height, size_t p, bool* in )
{
    const long long qx = ( long long )x + dx, qy = ( long long )y + dy;
    *in = qx >= 0 && qx < ( long long )width && qy >= 0 && qy < ( long long )height;
    return *in ? ( size_t )qy * width + ( size_t )qx : p;
}

#endif
