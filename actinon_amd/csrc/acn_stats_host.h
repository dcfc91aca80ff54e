/* acn_stats_host.h -- the host-side checks of the lens and lens-statistics entry points that need neither a handle nor the GPU:
 * plain C++, no HIP.  acn_calls.hip calls them before it touches a handle; tests/csrc/stats_cpu.cpp compiles them on their own
 * into a program that runs under the address and undefined-behaviour sanitizers.  Each returns an acn_status and, on a refusal, the
 * message acn_last_error will carry. */
#ifndef ACN_STATS_HOST_H
#define ACN_STATS_HOST_H

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "actinon_hip.h"

/* an acn_lens_params as far as the caller's header knew it (struct_size), the rest zero; null is ACN_LENS_PARAMS_INIT.  Then the checks
 * of the members alone, in the order the header lists them */
static inline int acn_lens_params_read( const acn_lens_params* prm, acn_lens_params* out, std::string* msg )
{
    acn_lens_params p = ACN_LENS_PARAMS_INIT;
    if( prm )
    {
        if( prm->struct_size < sizeof( uint32_t ) ) { *msg = "acn_lens_params.struct_size " + std::to_string( prm->struct_size ) + " is smaller than its first member"; return ACN_ERR_ARG; }
        p = acn_lens_params{};
        memcpy( &p, prm, prm->struct_size < sizeof( p ) ? prm->struct_size : sizeof( p ) );
    }
    if( p.samples > ACN_LENS_MAX_SAMPLES ) { *msg = "acn_lens_params.samples " + std::to_string( p.samples ) + " is above 4096"; return ACN_ERR_ARG; }
    if( p.flags & ~ACN_LENS_JITTER ) { *msg = "unknown acn_lens_params.flags bits"; return ACN_ERR_ARG; }
    if( !( p.aperture_radius >= 0 ) || p.aperture_radius > 1.7976931348623157e308 ) { *msg = "acn_lens_params.aperture_radius is negative or not finite"; return ACN_ERR_ARG; }
    if( p.aperture_radius > 0 && !( p.focus_distance > 0 && p.focus_distance <= 1.7976931348623157e308 ) )
    {
        *msg = "acn_lens_params.focus_distance must be positive and finite when the aperture is open";
        return ACN_ERR_ARG;
    }
    *out = p;
    return ACN_OK;
}

/* the indices of acn_lens_stats_merge (host form): without an index the part must fit the accumulator; with one, every index lies in
 * [ 0, n_acc ) and none comes twice */
static inline int acn_stats_index_check( const int64_t* index, size_t n_part, size_t n_acc, std::string* msg )
{
    if( !index )
    {
        if( n_part > n_acc ) { *msg = "a merge without an index needs n_part <= n_acc: " + std::to_string( n_part ) + " records for " + std::to_string( n_acc ); return ACN_ERR_ARG; }
        return ACN_OK;
    }
    std::vector< bool > seen( n_acc, false );
    for( size_t j = 0; j < n_part; j++ )
    {
        const int64_t i = index[ j ];
        if( i < 0 || ( uint64_t )i >= ( uint64_t )n_acc )
        {
            *msg = "index[ " + std::to_string( j ) + " ] = " + std::to_string( ( long long )i ) + " is out of range: the accumulator has " + std::to_string( n_acc ) + " records";
            return ACN_ERR_ARG;
        }
        if( seen[ ( size_t )i ] ) { *msg = "index[ " + std::to_string( j ) + " ] = " + std::to_string( ( long long )i ) + " is a duplicate"; return ACN_ERR_ARG; }
        seen[ ( size_t )i ] = true;
    }
    return ACN_OK;
}

/* a buffer of statistics records: read and written 16 bytes at a time */
static inline int acn_stats_buffer_check( const void* stats, size_t n, const char* what, std::string* msg )
{
    if( n && !stats ) { *msg = std::string( "null argument: " ) + what; return ACN_ERR_ARG; }
    if( ( uintptr_t )stats % 16 ) { *msg = std::string( what ) + " is read and written 16 bytes at a time: align the buffer"; return ACN_ERR_ARG; }
    if( n > ( ( size_t )1 << 38 ) ) { *msg = std::string( what ) + ": too many records in one call"; return ACN_ERR_ARG; }
    return ACN_OK;
}

#endif
