/* acn_select_host.h -- what acn_select_above* and acn_key_histogram* do without a handle and without the GPU: the reading of
 * acn_select_params, every argument check of the two calls, the bin of a key, acn_key_hist_edge and acn_key_hist_threshold.  Plain
 * C++, no HIP header: acn_calls.hip calls these before it touches a handle, k_select.hip compiles the bin function for the device
 * as well (the one expression both sides use), and tests/csrc/select_cpu.cpp compiles the header on its own, as a shim for the
 * CPU tests and as a program that runs under the address and undefined-behaviour sanitizers.  A check returns an acn_status and, on
 * a refusal, the message acn_last_error will carry. */
#ifndef ACN_SELECT_HOST_H
#define ACN_SELECT_HOST_H

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>

#include "actinon_hip.h"

#if defined( __HIPCC__ )
#define ACN_SELECT_HD __host__ __device__
#else
#define ACN_SELECT_HD
#endif

/* entries of one tile of the select kernels: a power of two in [ 256, 8192 ], a multiple of the 256 lanes of a workgroup */
#define ACN_SELECT_TILE 2048u
#define ACN_SELECT_MAX_N ( ( uint64_t )1 << 31 )
/* positions of a raster are exact in binary64 below this pixel number */
#define ACN_SELECT_MAX_PIXEL ( ( uint64_t )1 << 52 )
#define ACN_KEY_HIST_LO ( ( 1023u - 40u ) * 4u )

static inline uint64_t acn_select_tiles( uint64_t n ) { return ( n + ( ACN_SELECT_TILE - 1 ) ) / ACN_SELECT_TILE; }

/* the histogram word of a key with the raw bits u (include/actinon_hip.h, ACN_KEY_HIST_*) */
ACN_SELECT_HD static inline uint32_t acn_select_key_bin( uint64_t u )
{
    if( ( u & 0x7FFFFFFFFFFFFFFFull ) > 0x7FF0000000000000ull ) return 256u;   /* NaN, either sign */
    if( u >> 63 ) return 0u;                                                    /* negative, -0.0 and -inf included */
    const uint32_t e = ( uint32_t )( u >> 50 );                                 /* exponent and the two top mantissa bits */
    if( e < ACN_KEY_HIST_LO ) return 0u;
    const uint32_t b = e - ACN_KEY_HIST_LO + 1u;
    return b < 255u ? b : 255u;
}

static inline double acn_select_bits_double( uint64_t u ) { double d; memcpy( &d, &u, sizeof( d ) ); return d; }

/* the lower edge of bin j: -inf for bin 0, NaN above 255 */
static inline double acn_select_hist_edge( uint32_t bin )
{
    if( bin == 0 ) return acn_select_bits_double( 0xFFF0000000000000ull );
    if( bin > 255 ) return acn_select_bits_double( 0x7FF8000000000000ull );
    return acn_select_bits_double( ( uint64_t )( ACN_KEY_HIST_LO + bin - 1u ) << 50 );
}

/* edge( j ) of the smallest j >= 1 with hist[ j ] + ... + hist[ 255 ] <= budget, +inf if there is none; a null hist gives NaN */
static inline double acn_select_hist_threshold( const uint64_t* hist, uint64_t budget )
{
    if( !hist ) return acn_select_bits_double( 0x7FF8000000000000ull );
    uint64_t above = 0;       /* hist[ j ] + ... + hist[ 255 ] */
    uint32_t j = 256;         /* the smallest bin known to fit; 256: none yet */
    while( j > 1 )
    {
        const uint64_t c = hist[ j - 1 ];
        if( above + c < above ) break;   /* (a sum past 2^64 is above every budget) */
        above += c;
        if( above > budget ) break;
        j--;
    }
    return j > 255 ? acn_select_bits_double( 0x7FF0000000000000ull ) : acn_select_hist_edge( j );
}

/* an acn_select_params as far as the caller's header knew it (struct_size), the rest zero, then the checks of the members alone */
static inline int acn_select_params_read( const acn_select_params* prm, acn_select_params* out, std::string* msg )
{
    if( !prm ) { *msg = "null argument: acn_select_params (the threshold has no default)"; return ACN_ERR_ARG; }
    uint32_t size;
    memcpy( &size, prm, sizeof( size ) );
    if( size < 16 ) { *msg = "acn_select_params.struct_size " + std::to_string( size ) + " does not reach the threshold (16 bytes)"; return ACN_ERR_ARG; }
    acn_select_params p{};
    memcpy( &p, prm, size < sizeof( p ) ? size : sizeof( p ) );
    if( p.flags ) { *msg = "unknown acn_select_params.flags bits"; return ACN_ERR_ARG; }
    if( p.threshold != p.threshold ) { *msg = "acn_select_params.threshold is NaN"; return ACN_ERR_ARG; }
    *out = p;
    return ACN_OK;
}

/* every check of acn_select_above* that needs no handle, in the order the header lists them; *out: the parameters as read */
static inline int acn_select_args_check( bool have_handle, const void* key, uint64_t n, const acn_select_params* prm, const void* src_pos_xy,
                                         const void* out_index, const void* out_pos_xy, uint32_t shard_world, acn_select_params* out,
                                         std::string* msg )
{
    if( !have_handle ) { *msg = "null argument: handle"; return ACN_ERR_ARG; }
    if( n && !key ) { *msg = "null argument: key"; return ACN_ERR_ARG; }
    if( n > ACN_SELECT_MAX_N ) { *msg = "n " + std::to_string( n ) + " is above 2^31 entries in one select call"; return ACN_ERR_ARG; }
    const int st = acn_select_params_read( prm, out, msg );
    if( st != ACN_OK ) return st;
    if( out->capacity && !out_index && !out_pos_xy ) { *msg = "null argument: capacity " + std::to_string( out->capacity ) + " with neither out_index nor out_pos_xy"; return ACN_ERR_ARG; }
    if( shard_world > 1 ) { *msg = "a select call is not sharded"; return ACN_ERR_ARG; }
    if( ( uintptr_t )key % 8 || ( uintptr_t )src_pos_xy % 8 || ( uintptr_t )out_index % 8 || ( uintptr_t )out_pos_xy % 8 )
    {
        *msg = "the buffers of a select call hold 8-byte entries: align them";
        return ACN_ERR_ARG;
    }
    if( !src_pos_xy && out_pos_xy && ( out->raster_first > ACN_SELECT_MAX_PIXEL || n > ACN_SELECT_MAX_PIXEL - out->raster_first ) )
    {
        *msg = "raster_first + n is above 2^52: the pixel centres would not be exact";
        return ACN_ERR_ARG;
    }
    return ACN_OK;
}

/* every check of acn_key_histogram* that needs no handle */
static inline int acn_key_hist_args_check( bool have_handle, const void* key, uint64_t n, const void* out_hist, uint32_t shard_world, std::string* msg )
{
    if( !have_handle ) { *msg = "null argument: handle"; return ACN_ERR_ARG; }
    if( n && !key ) { *msg = "null argument: key"; return ACN_ERR_ARG; }
    if( !out_hist ) { *msg = "null argument: out_hist"; return ACN_ERR_ARG; }
    if( n > ACN_SELECT_MAX_N ) { *msg = "n " + std::to_string( n ) + " is above 2^31 entries in one histogram call"; return ACN_ERR_ARG; }
    if( shard_world > 1 ) { *msg = "a histogram call is not sharded"; return ACN_ERR_ARG; }
    if( ( uintptr_t )key % 8 || ( uintptr_t )out_hist % 8 ) { *msg = "the buffers of a histogram call hold 8-byte entries: align them"; return ACN_ERR_ARG; }
    return ACN_OK;
}

#endif
