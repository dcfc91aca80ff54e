/* acn_reproject_host.h -- what acn_reproject* checks without a handle and without the GPU.  Plain C++, no HIP header: acn_calls.hip calls
 * these before it touches a handle; tests/csrc/reproject_cpu.cpp compiles the header on its own into a program that runs under the
 * address and undefined-behaviour sanitizers.  A check returns an acn_status and, on a refusal, the message acn_last_error will
 * carry.  What acn_scene_set_params refuses of the previous frame's parameters beyond the raster (acn_tables_validate_params) stays
 * with acn_calls.hip, which has that unit. */
#ifndef ACN_REPROJECT_HOST_H
#define ACN_REPROJECT_HOST_H

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>

#include "actinon_hip.h"

#define ACN_REPROJECT_MAX_N ( ( uint64_t )1 << 31 )

/* an acn_reproject_params as far as the caller's header knew it (struct_size), the rest zero; null is ACN_REPROJECT_PARAMS_INIT.  Then
 * the checks of the members in the order the header lists them.  *out: every member at its final value, no default left */
static inline int acn_reproject_params_read( const acn_reproject_params* prm, acn_reproject_params* out, std::string* msg )
{
    acn_reproject_params p = ACN_REPROJECT_PARAMS_INIT;
    if( prm )
    {
        if( prm->struct_size < sizeof( uint32_t ) ) { *msg = "acn_reproject_params.struct_size " + std::to_string( prm->struct_size ) + " is smaller than its first member"; return ACN_ERR_ARG; }
        p = acn_reproject_params{};
        memcpy( &p, prm, prm->struct_size < sizeof( p ) ? prm->struct_size : sizeof( p ) );
    }
    const double dbl_max = 1.7976931348623157e308;
    if( p.flags & ~( ACN_REPROJECT_KINDS_SET | ACN_REPROJECT_HOPS_SET ) ) { *msg = "unknown acn_reproject_params.flags bits"; return ACN_ERR_ARG; }
    if( !( p.normal_min >= -1.0 && p.normal_min <= 1.0 ) ) { *msg = "acn_reproject_params.normal_min is outside [ -1, 1 ]"; return ACN_ERR_ARG; }
    if( !( p.plane_tolerance >= 0 ) || p.plane_tolerance > dbl_max ) { *msg = "acn_reproject_params.plane_tolerance is negative or not finite"; return ACN_ERR_ARG; }
    if( p.max_history != 0 && !( p.max_history >= 1.0 && p.max_history <= dbl_max ) ) { *msg = "acn_reproject_params.max_history is not a finite number >= 1"; return ACN_ERR_ARG; }
    if( !( p.flags & ACN_REPROJECT_KINDS_SET ) && p.reject_kinds == 0 ) p.reject_kinds = ACN_REPROJECT_DEFAULT_REJECT_KINDS;
    if( !( p.flags & ACN_REPROJECT_HOPS_SET ) && p.max_hops == 0 ) p.max_hops = ACN_REPROJECT_DEFAULT_MAX_HOPS;
    if( p.normal_min == 0 ) p.normal_min = ACN_REPROJECT_DEFAULT_NORMAL_MIN;
    if( p.plane_tolerance == 0 ) p.plane_tolerance = ACN_REPROJECT_DEFAULT_PLANE_TOLERANCE;
    if( p.max_history == 0 ) p.max_history = ACN_REPROJECT_DEFAULT_MAX_HISTORY;
    *out = p;
    return ACN_OK;
}

/* every check of acn_reproject* that needs no handle, in the order the header lists them; *out_prm: the parameters as read */
static inline int acn_reproject_check( bool have_handle, const void* cur_surface, uint64_t n, const acn_params* prev_params, const void* prev_surface,
                                       const void* prev_stats, const acn_reproject_params* prm, const void* out_stats, const void* out_motion,
                                       uint32_t shard_world, acn_reproject_params* out_prm, std::string* msg )
{
    if( !have_handle ) { *msg = "null argument: handle"; return ACN_ERR_ARG; }
    if( !prev_params ) { *msg = "null argument: prev_params"; return ACN_ERR_ARG; }
    if( n && !cur_surface ) { *msg = "null argument: cur_surface"; return ACN_ERR_ARG; }
    if( n && !prev_surface ) { *msg = "null argument: prev_surface"; return ACN_ERR_ARG; }
    if( n && !prev_stats ) { *msg = "null argument: prev_stats"; return ACN_ERR_ARG; }
    if( n && !out_stats ) { *msg = "null argument: out_stats"; return ACN_ERR_ARG; }
    if( n > ACN_REPROJECT_MAX_N ) { *msg = "n " + std::to_string( n ) + " is above 2^31 positions in one call"; return ACN_ERR_ARG; }
    const uint64_t w = prev_params->image_width, h = prev_params->image_height;
    if( h < 2 || w < 1 ) { *msg = "the previous raster needs a width and a height of at least 2"; return ACN_ERR_ARG; }
    if( w > ACN_REPROJECT_MAX_N || h > ACN_REPROJECT_MAX_N || w * h > ACN_REPROJECT_MAX_N ) { *msg = "the previous raster has more than 2^31 pixels"; return ACN_ERR_ARG; }
    if( ( uintptr_t )cur_surface % 16 || ( uintptr_t )prev_surface % 16 || ( uintptr_t )prev_stats % 16 || ( uintptr_t )out_stats % 16 )
    {
        *msg = "surface and statistics records are read and written 16 bytes at a time: align the buffers";
        return ACN_ERR_ARG;
    }
    if( ( uintptr_t )out_motion % 8 ) { *msg = "out_motion is an array of doubles: align the buffer"; return ACN_ERR_ARG; }
    const int st = acn_reproject_params_read( prm, out_prm, msg );
    if( st != ACN_OK ) return st;
    if( shard_world > 1 ) { *msg = "a reproject call is not sharded: slice the list of positions"; return ACN_ERR_ARG; }
    return ACN_OK;
}

#endif
