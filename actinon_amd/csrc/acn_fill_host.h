/* acn_fill_host.h -- every check of an acn_fill_stats* call and the reading of its acn_fill_params, none of which needs a handle or
 * the GPU: plain C++, no HIP.  acn_calls.hip calls acn_fill_check before it touches a handle; tests/csrc/fill_cpu.cpp compiles it on
 * its own behind a shim that tests/test_fill_cpu.py loads.  Returns an acn_status and, on a refusal, the message acn_last_error
 * will carry. */
#ifndef ACN_FILL_HOST_H
#define ACN_FILL_HOST_H

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>

#include "actinon_hip.h"

/* the parameters of a call as the kernels take them: final values, no defaults */
struct FillSetup { uint32_t radius, normal_power_log2, no_demodulate; double sigma_px, sigma_plane; };

/* [ a, a + a_bytes ) and [ b, b + b_bytes ) share a byte */
static inline bool acn_fill_overlap( const void* a, size_t a_bytes, const void* b, size_t b_bytes )
{
    const uintptr_t a0 = ( uintptr_t )a, b0 = ( uintptr_t )b;
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

/* have_handle: the caller's handle is not null (the one thing of it that is checked here) */
static inline int acn_fill_check( bool have_handle, const void* stats, const void* surface, size_t width, size_t height, const acn_fill_params* prm,
                                  const void* out_stats, const void* out_need, uint32_t shard_world, FillSetup* su, std::string* msg )
{
    if( !have_handle || !stats || !surface || !out_stats ) { *msg = "null argument"; return ACN_ERR_ARG; }
    const size_t max_n = ( size_t )1 << 31;
    if( width == 0 || height == 0 ) { *msg = "a frame to fill needs a width and a height"; return ACN_ERR_ARG; }
    if( width > max_n || height > max_n || width * height > max_n ) { *msg = "a frame to fill has at most 2^31 pixels"; return ACN_ERR_ARG; }
    acn_fill_params p{};
    if( prm )
    {
        if( prm->struct_size < sizeof( uint32_t ) ) { *msg = "acn_fill_params.struct_size " + std::to_string( prm->struct_size ) + " is smaller than its first member"; return ACN_ERR_ARG; }
        memcpy( &p, prm, prm->struct_size < sizeof( p ) ? prm->struct_size : sizeof( p ) );
    }
    if( p.flags & ~( ACN_DENOISE_NO_DEMODULATE | ACN_DENOISE_NORMAL_POWER_SET ) ) { *msg = "unknown acn_fill_params.flags bits"; return ACN_ERR_ARG; }
    if( p.radius > ACN_FILL_MAX_RADIUS ) { *msg = "acn_fill_params.radius " + std::to_string( p.radius ) + " is above 8"; return ACN_ERR_ARG; }
    if( p.normal_power_log2 > ACN_DENOISE_MAX_NORMAL_POWER_LOG2 ) { *msg = "acn_fill_params.normal_power_log2 " + std::to_string( p.normal_power_log2 ) + " is above 10"; return ACN_ERR_ARG; }
    const double sig[ 2 ] = { p.sigma_px, p.sigma_plane };
    for( double s : sig ) if( !( s >= 0 ) || s > 1.7976931348623157e308 ) { *msg = "a sigma of acn_fill_params is negative or not finite"; return ACN_ERR_ARG; }
    if( shard_world > 1 ) { *msg = "a fill call is not sharded: the gather needs the whole frame"; return ACN_ERR_ARG; }
    if( ( uintptr_t )stats % 16 || ( uintptr_t )out_stats % 16 ) { *msg = "statistics records are read and written 16 bytes at a time: align stats and out_stats"; return ACN_ERR_ARG; }
    if( ( uintptr_t )surface % 16 ) { *msg = "the surface records of a fill call are read 16 bytes at a time: align the buffer"; return ACN_ERR_ARG; }
    if( ( uintptr_t )out_need % 8 ) { *msg = "out_need holds doubles: align the buffer"; return ACN_ERR_ARG; }
    const size_t n = width * height, rec_bytes = n * ACN_STATS_STRIDE * sizeof( double ), need_bytes = n * sizeof( double );
    if( acn_fill_overlap( stats, rec_bytes, out_stats, rec_bytes ) ) { *msg = "out_stats overlaps stats: the gather reads its neighbours' inputs"; return ACN_ERR_ARG; }
    if( out_need && ( acn_fill_overlap( stats, rec_bytes, out_need, need_bytes ) || acn_fill_overlap( out_stats, rec_bytes, out_need, need_bytes ) ) )
    {
        *msg = "out_need overlaps stats or out_stats";
        return ACN_ERR_ARG;
    }
    su->radius = p.radius ? p.radius : ACN_FILL_DEFAULT_RADIUS;
    su->normal_power_log2 = ( p.normal_power_log2 || ( p.flags & ACN_DENOISE_NORMAL_POWER_SET ) ) ? p.normal_power_log2 : ACN_DENOISE_DEFAULT_NORMAL_POWER_LOG2;
    su->no_demodulate = ( p.flags & ACN_DENOISE_NO_DEMODULATE ) ? 1u : 0u;
    su->sigma_px = p.sigma_px != 0 ? p.sigma_px : ACN_FILL_DEFAULT_SIGMA_PX;
    su->sigma_plane = p.sigma_plane != 0 ? p.sigma_plane : ACN_FILL_DEFAULT_SIGMA_PLANE;
    return ACN_OK;
}

#endif
