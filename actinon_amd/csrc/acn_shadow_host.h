/* acn_shadow_host.h -- what acn_shadow_records* and acn_shadow_limit_history* check without a handle and without the GPU.  Plain C++,
 * no HIP header, in the manner of acn_reproject_host.h: acn_calls.hip calls these before it touches a handle.  A check returns an
 * acn_status and, on a refusal, the message acn_last_error will carry. */
#ifndef ACN_SHADOW_HOST_H
#define ACN_SHADOW_HOST_H

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>

#include "actinon_hip.h"

#define ACN_SHADOW_MAX_N ( ( uint64_t )1 << 31 )

/* an acn_shadow_params as far as the caller's header knew it (struct_size), the rest zero; null is ACN_SHADOW_PARAMS_INIT.
 * *log2_samples: S = 1 << *log2_samples, the default applied */
static inline int acn_shadow_params_read( const acn_shadow_params* prm, uint32_t* log2_samples, std::string* msg )
{
    acn_shadow_params p = ACN_SHADOW_PARAMS_INIT;
    if( prm )
    {
        if( prm->struct_size < sizeof( uint32_t ) ) { *msg = "acn_shadow_params.struct_size " + std::to_string( prm->struct_size ) + " is smaller than its first member"; return ACN_ERR_ARG; }
        p = acn_shadow_params{};
        memcpy( &p, prm, prm->struct_size < sizeof( p ) ? prm->struct_size : sizeof( p ) );
    }
    if( p.flags ) { *msg = "unknown acn_shadow_params.flags bits"; return ACN_ERR_ARG; }
    const uint32_t s = p.samples == 0 ? ( uint32_t )ACN_SHADOW_DEFAULT_SAMPLES : p.samples;
    if( s > ACN_SHADOW_MAX_SAMPLES || ( s & ( s - 1u ) ) ) { *msg = "acn_shadow_params.samples " + std::to_string( s ) + " is not 1, 2, 4, 8, 16, 32 or 64"; return ACN_ERR_ARG; }
    uint32_t l = 0;
    while( ( 1u << l ) < s ) l++;
    *log2_samples = l;
    return ACN_OK;
}

/* every check of acn_shadow_records* that needs no handle, in the order the header lists them */
static inline int acn_shadow_records_check( bool have_handle, const void* surface, uint64_t n, const acn_shadow_params* prm, const void* out,
                                            uint32_t shard_world, uint32_t* log2_samples, std::string* msg )
{
    if( !have_handle ) { *msg = "null argument: handle"; return ACN_ERR_ARG; }
    if( n && !surface ) { *msg = "null argument: surface"; return ACN_ERR_ARG; }
    if( n && !out ) { *msg = "null argument: out"; return ACN_ERR_ARG; }
    if( n > ACN_SHADOW_MAX_N ) { *msg = "n " + std::to_string( n ) + " is above 2^31 positions in one call"; return ACN_ERR_ARG; }
    if( ( uintptr_t )surface % 16 || ( uintptr_t )out % 16 ) { *msg = "surface and shadow records are read and written 16 bytes at a time: align the buffers"; return ACN_ERR_ARG; }
    const int st = acn_shadow_params_read( prm, log2_samples, msg );
    if( st != ACN_OK ) return st;
    if( shard_world > 1 ) { *msg = "a shadow call is not sharded: slice the list of positions"; return ACN_ERR_ARG; }
    return ACN_OK;
}

/* the same for acn_shadow_history_params; *out: every member at its final value, no default left */
static inline int acn_shadow_history_params_read( const acn_shadow_history_params* prm, acn_shadow_history_params* out, std::string* msg )
{
    acn_shadow_history_params p = ACN_SHADOW_HISTORY_PARAMS_INIT;
    if( prm )
    {
        if( prm->struct_size < sizeof( uint32_t ) ) { *msg = "acn_shadow_history_params.struct_size " + std::to_string( prm->struct_size ) + " is smaller than its first member"; return ACN_ERR_ARG; }
        p = acn_shadow_history_params{};
        memcpy( &p, prm, prm->struct_size < sizeof( p ) ? prm->struct_size : sizeof( p ) );
    }
    const double dbl_max = 1.7976931348623157e308;
    if( p.flags & ~ACN_SHADOW_HISTORY_DROP ) { *msg = "unknown acn_shadow_history_params.flags bits"; return ACN_ERR_ARG; }
    if( !( p.tolerance >= 0 ) || p.tolerance > dbl_max ) { *msg = "acn_shadow_history_params.tolerance is negative or not finite"; return ACN_ERR_ARG; }
    if( p.changed_max_history != 0 && !( p.changed_max_history >= 1.0 && p.changed_max_history <= dbl_max ) ) { *msg = "acn_shadow_history_params.changed_max_history is not a finite number >= 1"; return ACN_ERR_ARG; }
    if( p.tolerance == 0 ) p.tolerance = ACN_SHADOW_HISTORY_DEFAULT_TOLERANCE;
    if( p.changed_max_history == 0 ) p.changed_max_history = ACN_SHADOW_HISTORY_DEFAULT_MAX_HISTORY;
    *out = p;
    return ACN_OK;
}

/* every check of acn_shadow_limit_history* that needs no handle, in the order the header lists them */
static inline int acn_shadow_limit_history_check( bool have_handle, const void* stats, const void* motion, const void* cur_shadow, const void* prev_shadow,
                                                  uint64_t n, uint64_t width, uint64_t height, const acn_shadow_history_params* prm,
                                                  const void* out_change, uint32_t shard_world, acn_shadow_history_params* out_prm, std::string* msg )
{
    if( !have_handle ) { *msg = "null argument: handle"; return ACN_ERR_ARG; }
    if( n && !stats ) { *msg = "null argument: stats"; return ACN_ERR_ARG; }
    if( n && !motion ) { *msg = "null argument: motion"; return ACN_ERR_ARG; }
    if( n && !cur_shadow ) { *msg = "null argument: cur_shadow"; return ACN_ERR_ARG; }
    if( n && !prev_shadow ) { *msg = "null argument: prev_shadow"; return ACN_ERR_ARG; }
    if( n > ACN_SHADOW_MAX_N ) { *msg = "n " + std::to_string( n ) + " is above 2^31 positions in one call"; return ACN_ERR_ARG; }
    if( width < 1 || height < 1 ) { *msg = "the previous raster needs a width and a height of at least 1"; return ACN_ERR_ARG; }
    if( width > ACN_SHADOW_MAX_N || height > ACN_SHADOW_MAX_N || width * height > ACN_SHADOW_MAX_N ) { *msg = "the previous raster has more than 2^31 pixels"; return ACN_ERR_ARG; }
    if( ( uintptr_t )stats % 16 || ( uintptr_t )cur_shadow % 16 || ( uintptr_t )prev_shadow % 16 )
    {
        *msg = "statistics and shadow records are read and written 16 bytes at a time: align the buffers";
        return ACN_ERR_ARG;
    }
    if( ( uintptr_t )motion % 8 || ( uintptr_t )out_change % 8 ) { *msg = "motion and out_change are arrays of doubles: align the buffers"; return ACN_ERR_ARG; }
    const int st = acn_shadow_history_params_read( prm, out_prm, msg );
    if( st != ACN_OK ) return st;
    if( shard_world > 1 ) { *msg = "a shadow call is not sharded: slice the list of positions"; return ACN_ERR_ARG; }
    return ACN_OK;
}

#endif
