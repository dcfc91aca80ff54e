/* acn_layers_host.h -- what acn_lens_layers_reduce*, acn_render_lens_layers*, acn_denoise_layers*, acn_lens_layers_merge* and
 * acn_lens_layers_resolve_dev check without a handle and without the GPU.  Plain C++, no HIP header: acn_calls.hip calls these before
 * it touches a handle; tests/csrc/layers_cpu.cpp and tests/csrc/layers_merge_cpu.cpp compile the header on its own into programs
 * that run under the address and undefined-behaviour sanitizers.  A check returns an acn_status
 * and, on a refusal, the message acn_last_error will carry.  What needs the handle's scene (an open aperture without a focal
 * length, a pixel range outside the image) and the parameters of the filter (denoise_check) stay with acn_calls.hip. */
#ifndef ACN_LAYERS_HOST_H
#define ACN_LAYERS_HOST_H

#include <cstddef>
#include <cstdint>
#include <string>

#include "acn_lenssurf_host.h"

/* every check of acn_lens_layers_reduce*, in the order the header lists them */
static inline int acn_layers_reduce_check( bool have_handle, const void* records, const void* radiance, uint64_t n, uint32_t K, const void* out_surface,
                                           const void* out_stats, uint32_t shard_world, std::string* msg )
{
    if( !have_handle ) { *msg = "null argument: handle"; return ACN_ERR_ARG; }
    if( n && !records ) { *msg = "null argument: records"; return ACN_ERR_ARG; }
    if( n && !radiance ) { *msg = "null argument: radiance"; return ACN_ERR_ARG; }
    if( n && !out_surface ) { *msg = "null argument: out_surface"; return ACN_ERR_ARG; }
    if( n && !out_stats ) { *msg = "null argument: out_stats"; return ACN_ERR_ARG; }
    if( K == 0 || K > ACN_LENS_MAX_SAMPLES ) { *msg = "K " + std::to_string( K ) + " samples per position: 1 .. 4096 are split"; return ACN_ERR_ARG; }
    if( shard_world > 1 ) { *msg = "a layers reduce call is not sharded: slice the array"; return ACN_ERR_ARG; }
    if( ( uintptr_t )records % 16 || ( uintptr_t )out_surface % 16 || ( uintptr_t )out_stats % 16 ) { *msg = "surface and statistics records are read and written 16 bytes at a time: align the buffers"; return ACN_ERR_ARG; }
    if( ( uintptr_t )radiance % 8 ) { *msg = "radiance is an array of doubles: align the buffer"; return ACN_ERR_ARG; }
    if( n > ACN_LENSSURF_MAX_N ) { *msg = "n " + std::to_string( n ) + " is above 2^38 positions in one call"; return ACN_ERR_ARG; }
    return ACN_OK;
}

/* every check of acn_render_lens_layers* that needs no handle: those of acn_surface_lens* and of acn_render_lens_stats* together.
 * need_pos: the call takes positions (not the main-pass form).  shard_*: of the call's acn_render_opts.  out_rgb is nullable
 * and not checked.  *out_prm: the parameters as read (a null prm is ACN_LENS_PARAMS_INIT) */
static inline int acn_layers_lens_check( bool have_handle, bool need_pos, const void* pos_xy, uint64_t n, const acn_lens_params* prm, uint32_t mode,
                                         const void* out_surface, const void* out_stats, uint32_t shard_mode, uint32_t shard_rank,
                                         uint32_t shard_world, acn_lens_params* out_prm, std::string* msg )
{
    if( !have_handle ) { *msg = "null argument: handle"; return ACN_ERR_ARG; }
    if( n && need_pos && !pos_xy ) { *msg = "null argument: pos_xy"; return ACN_ERR_ARG; }
    if( n && !out_surface ) { *msg = "null argument: out_surface"; return ACN_ERR_ARG; }
    if( n && !out_stats ) { *msg = "null argument: out_stats"; return ACN_ERR_ARG; }
    const int st = acn_lens_params_read( prm, out_prm, msg );
    if( st != ACN_OK ) return st;
    if( mode != ACN_SURF_FIRST_HIT && mode != ACN_SURF_FOLLOW ) { *msg = "unknown surface mode " + std::to_string( mode ); return ACN_ERR_ARG; }
    if( shard_mode > ACN_SHARD_SAMPLES ) { *msg = "unknown shard_mode"; return ACN_ERR_ARG; }
    if( shard_mode == ACN_SHARD_SAMPLES && shard_world > 1 )
    {
        if( shard_rank >= shard_world ) { *msg = "shard_rank >= shard_world"; return ACN_ERR_ARG; }
        *msg = "layered lens statistics are not sharded by samples (ACN_SHARD_SAMPLES): deviations of partial radiances mean nothing";
        return ACN_ERR_ARG;
    }
    if( ( need_pos && ( uintptr_t )pos_xy % 16 ) || ( uintptr_t )out_surface % 16 || ( uintptr_t )out_stats % 16 ) { *msg = "positions, surface and statistics records are moved 16 bytes at a time: align the buffers"; return ACN_ERR_ARG; }
    if( n > ACN_LENSSURF_MAX_N ) { *msg = "n " + std::to_string( n ) + " is above 2^38 positions in one call"; return ACN_ERR_ARG; }
    return ACN_OK;
}

/* the buffers of acn_denoise_layers* beyond what acn_denoise_stats* checks of its own: both are read 16 bytes at a time */
static inline int acn_layers_denoise_check( const void* stats, const void* surface, std::string* msg )
{
    if( ( uintptr_t )stats % 16 ) { *msg = "the statistics planes of a layered denoise call are read 16 bytes at a time: align the buffer"; return ACN_ERR_ARG; }
    if( ( uintptr_t )surface % 16 ) { *msg = "the surface planes of a layered denoise call are read 16 bytes at a time: align the buffer"; return ACN_ERR_ARG; }
    return ACN_OK;
}

/* every check of acn_lens_layers_merge* that needs no handle, in the order the header lists them.  index_is_host: the host form, whose
 * index list is read here -- acn_stats_index_check, as for acn_lens_stats_merge: in range and none twice --; the _dev form's list is
 * on the device, and only its alignment is checked */
static inline int acn_layers_merge_check( bool have_handle, const void* acc_surface, const void* acc_stats, uint64_t n_acc, const void* part_surface,
                                          const void* part_stats, uint64_t n_part, const int64_t* index, bool index_is_host, uint32_t shard_world,
                                          std::string* msg )
{
    if( !have_handle ) { *msg = "null argument: handle"; return ACN_ERR_ARG; }
    if( n_acc && !acc_surface ) { *msg = "null argument: acc_surface"; return ACN_ERR_ARG; }
    if( n_acc && !acc_stats ) { *msg = "null argument: acc_stats"; return ACN_ERR_ARG; }
    if( n_part && !part_surface ) { *msg = "null argument: part_surface"; return ACN_ERR_ARG; }
    if( n_part && !part_stats ) { *msg = "null argument: part_stats"; return ACN_ERR_ARG; }
    if( shard_world > 1 ) { *msg = "a merge of layered records is not sharded"; return ACN_ERR_ARG; }
    if( ( uintptr_t )acc_surface % 16 || ( uintptr_t )acc_stats % 16 || ( uintptr_t )part_surface % 16 || ( uintptr_t )part_stats % 16 )
    {
        *msg = "surface and statistics records are read and written 16 bytes at a time: align the buffers";
        return ACN_ERR_ARG;
    }
    if( ( uintptr_t )index % 8 ) { *msg = "index is an array of int64_t: align the buffer"; return ACN_ERR_ARG; }
    if( n_acc > ACN_LENSSURF_MAX_N || n_part > ACN_LENSSURF_MAX_N ) { *msg = "more than 2^38 positions in one call"; return ACN_ERR_ARG; }
    if( index_is_host || !index ) return acn_stats_index_check( index, ( size_t )n_part, ( size_t )n_acc, msg );
    return ACN_OK;
}

/* every check of acn_lens_layers_resolve_dev that needs no handle */
static inline int acn_layers_resolve_check( bool have_handle, const void* stats, uint64_t n, const void* out_rgb, const void* out_noise,
                                            const void* out_pooled, uint32_t shard_world, std::string* msg )
{
    if( !have_handle ) { *msg = "null argument: handle"; return ACN_ERR_ARG; }
    if( n && !stats ) { *msg = "null argument: stats"; return ACN_ERR_ARG; }
    if( shard_world > 1 ) { *msg = "a resolve of layered records is not sharded"; return ACN_ERR_ARG; }
    if( ( uintptr_t )stats % 16 || ( uintptr_t )out_pooled % 16 ) { *msg = "statistics records are read and written 16 bytes at a time: align the buffers"; return ACN_ERR_ARG; }
    if( ( uintptr_t )out_rgb % 8 || ( uintptr_t )out_noise % 8 ) { *msg = "out_rgb and out_noise are arrays of doubles: align the buffers"; return ACN_ERR_ARG; }
    if( n > ACN_LENSSURF_MAX_N ) { *msg = "n " + std::to_string( n ) + " is above 2^38 positions in one call"; return ACN_ERR_ARG; }
    return ACN_OK;
}

#endif
