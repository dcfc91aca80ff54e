/* acn_lenssurf_host.h -- what acn_surface_reduce* and acn_surface_lens* check without a handle and without the GPU, and the slice
 * arithmetic of a lens surface call.  Plain C++, no HIP header: acn_calls.hip calls these before it touches a handle;
 * tests/csrc/lenssurf_cpu.cpp compiles the header on its own into a program that runs under the address and undefined-behaviour
 * sanitizers.  A check returns an acn_status and, on a refusal, the message acn_last_error will carry.  What needs the handle's
 * scene (an open aperture without a focal length, a pixel range outside the image) stays with acn_calls.hip. */
#ifndef ACN_LENSSURF_HOST_H
#define ACN_LENSSURF_HOST_H

#include <cstddef>
#include <cstdint>
#include <string>

#include "acn_stats_host.h"

/* positions of one call: n * K * 128 bytes stays far below 2^64 */
#define ACN_LENSSURF_MAX_N ( ( uint64_t )1 << 38 )

/* every check of acn_surface_reduce*, in the order the header lists them */
static inline int acn_lenssurf_reduce_check( bool have_handle, const void* records, uint64_t n, uint32_t K, const void* out, uint32_t shard_world,
                                             std::string* msg )
{
    if( !have_handle ) { *msg = "null argument: handle"; return ACN_ERR_ARG; }
    if( n && !records ) { *msg = "null argument: records"; return ACN_ERR_ARG; }
    if( n && !out ) { *msg = "null argument: out"; return ACN_ERR_ARG; }
    if( K == 0 || K > ACN_LENS_MAX_SAMPLES ) { *msg = "K " + std::to_string( K ) + " records per position: 1 .. 4096 are reduced"; return ACN_ERR_ARG; }
    if( shard_world > 1 ) { *msg = "a surface reduce call is not sharded: slice the array"; return ACN_ERR_ARG; }
    if( ( uintptr_t )records % 16 || ( uintptr_t )out % 16 ) { *msg = "surface records are read and written 16 bytes at a time: align the buffers"; return ACN_ERR_ARG; }
    if( n > ACN_LENSSURF_MAX_N ) { *msg = "n " + std::to_string( n ) + " is above 2^38 positions in one call"; return ACN_ERR_ARG; }
    return ACN_OK;
}

/* every check of acn_surface_lens* that needs no handle.  need_pos: the call takes positions (not the main-pass form).  *out_prm: the
 * parameters as read (a null prm is ACN_LENS_PARAMS_INIT) */
static inline int acn_lenssurf_lens_check( bool have_handle, bool need_pos, const void* pos_xy, uint64_t n, const acn_lens_params* prm, uint32_t mode,
                                           const void* out, uint32_t shard_world, acn_lens_params* out_prm, std::string* msg )
{
    if( !have_handle ) { *msg = "null argument: handle"; return ACN_ERR_ARG; }
    if( n && need_pos && !pos_xy ) { *msg = "null argument: pos_xy"; return ACN_ERR_ARG; }
    if( n && !out ) { *msg = "null argument: out"; return ACN_ERR_ARG; }
    const int st = acn_lens_params_read( prm, out_prm, msg );
    if( st != ACN_OK ) return st;
    if( mode != ACN_SURF_FIRST_HIT && mode != ACN_SURF_FOLLOW ) { *msg = "unknown surface mode " + std::to_string( mode ); return ACN_ERR_ARG; }
    if( shard_world > 1 ) { *msg = "a lens surface call is not sharded: slice the array"; return ACN_ERR_ARG; }
    if( ( need_pos && ( uintptr_t )pos_xy % 16 ) || ( uintptr_t )out % 16 ) { *msg = "positions and surface records are moved 16 bytes at a time: align the buffers"; return ACN_ERR_ARG; }
    if( n > ACN_LENSSURF_MAX_N ) { *msg = "n " + std::to_string( n ) + " is above 2^38 positions in one call"; return ACN_ERR_ARG; }
    return ACN_OK;
}

/* positions of one slice of a lens call: floor( slice_rays / K ), at least 1, at most n (acn_render_lens* cut the same way) */
static inline size_t acn_lenssurf_slice( size_t slice_rays, uint32_t K, size_t n )
{
    size_t slice = K ? slice_rays / K : slice_rays;
    if( slice < 1 ) slice = 1;
    if( slice > n ) slice = n;
    return slice;
}

#endif
