/* acn_surfclass.h -- the class ( hit, e, x, h ) of a surface record as the kernels that reduce the K records of a position compare it
 * (k_lens_surface.hip, k_lens_layers.hip; include/actinon_hip.h states the class under acn_surface_reduce*). */
#ifndef ACN_SURFCLASS_H
#define ACN_SURFCLASS_H

#include <hip/hip_runtime.h>
#include <cstdint>

/* the class of a sample as two words: ( e, x ) and ( h, hit ) */
struct SurfKey { uint64_t ex, hh; };

__device__ static inline SurfKey surf_key( const double* r )
{
    SurfKey key;
    const uint32_t e = ( uint32_t )( int32_t )r[ 7 ], x = ( uint32_t )( int32_t )r[ 8 ], h = ( uint32_t )( int32_t )r[ 13 ];
    key.ex = ( ( uint64_t )e << 32 ) | x;
    key.hh = ( ( uint64_t )h << 1 ) | ( r[ 0 ] < __builtin_inf() ? 1u : 0u );
    return key;
}

__device__ static inline bool surf_key_eq( const SurfKey& a, const SurfKey& b ) { return a.ex == b.ex && a.hh == b.hh; }

#endif
