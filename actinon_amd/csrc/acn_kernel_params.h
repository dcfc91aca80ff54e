/* acn_kernel_params.h -- how a kernel receives the scene: the parameter and prologue macros of every kernel that takes SceneArgs
 * (the pipeline's, k_surface, k_query), and the occupancies the pipeline kernels are built for. */
#ifndef ACN_KERNEL_PARAMS_H
#define ACN_KERNEL_PARAMS_H

#include "acn_device.h"

#ifndef ACN_SHADE_WAVES
#define ACN_SHADE_WAVES 4
#endif
#ifndef ACN_WALK_WAVES
#define ACN_WALK_WAVES 4
#endif
/* Kernel parameter convention: every scene buffer is passed as its own __restrict__ pointer and the DevScene view is
 * rebuilt inside (scene arrays are then read through the constant address space, see acn_device.h); p_counts is the
 * counter block of the kernel's level. */
#define ACN_SCENE_PARAMS  DevScene sc_in, const GNode* __restrict__ p_nodes, const GMat* __restrict__ p_mats, const int32_t* __restrict__ p_elems, const acn_texture* __restrict__ p_textures
#define ACN_SCENE_VIEW    DevScene sc = sc_in; sc.nodes = ( NodeP )p_nodes; sc.gnodes = ( NodeP )p_nodes; sc.mats = ( MatP )p_mats; sc.elems = ( ElemP )p_elems; sc.textures = ( TexP )p_textures; sc.flags = sc_in.flags; sc.lds_stack = ACN_NO_LDS_STACK;

/* One ACN_FLAG_* word per chunk (DevScene.flags: the word of the chunk's first counter block), whatever the path level of
 * the kernel that raises a flag.  A queue that overflowed means the host will redo the chunk smaller (launch_render):
 * every later kernel of the chain, enqueued blind, looks at the word first and leaves at once -- the rest of a lost
 * chunk costs launches, not work (scenes with thousands of hits per position redo 15 - 25 % of their chunks). */
/* (the word is loaded next to the kernel's input count, one wait for both: a load of its own at the top of every kernel cost
 * 0.5 ms of the 71 ms frame, ~200 launches of which each is on the chunk's critical path) */
#define ACN_CHUNK_FLAGS_LOAD const uint32_t chunk_flags_ = *( const uint32_t* )sc_in.flags;
#define ACN_LEAVE_IF_CHUNK_IS_LOST \
    if( __builtin_amdgcn_readfirstlane( ( int )chunk_flags_ ) & ( int )ACN_FLAGS_CHUNK_LOST ) return;
/* The same for the kernels whose waves depend on each other afterwards (ACN_STAGE_NODES: every wave copies its quarter of the
 * node array into LDS, then the block synchronises).  Other workgroups of the SAME launch set the word concurrently, so the waves
 * of one workgroup may read different values; a wave that left alone would leave its quarter of the staged nodes unwritten and
 * the others would traverse garbage (a spurious ACN_FLAG_STACK_OVERFLOW turned a recoverable lost chunk into a failed call:
 * ADVICE r03).  Wave 0's reading decides for the whole workgroup. */
#define ACN_LEAVE_IF_CHUNK_IS_LOST_BLOCK \
    { \
        __shared__ uint32_t chunk_lost_; \
        if( threadIdx.x == 0 ) chunk_lost_ = chunk_flags_ & ACN_FLAGS_CHUNK_LOST; \
        __syncthreads(); \
        if( chunk_lost_ ) return; \
    }

/* LDS staging of the node array (kernels whose node reads are per-lane: the CSG machines).  The block copies the
 * GNode array into dynamic shared memory once; per-lane node reads then are ds_read instead of global loads. */
#define ACN_STAGE_NODES( sc ) \
    { \
        const double* src_ = ( const double* )p_nodes; \
        uint32_t words_ = ( sc ).n_nodes * ( uint32_t )( sizeof( GNode ) / sizeof( double ) ); \
        for( uint32_t k_ = threadIdx.x; k_ < words_; k_ += blockDim.x ) acn_lds_raw[ k_ ] = src_[ k_ ]; \
        __syncthreads(); \
    }

#ifndef ACN_TRACE_WAVES
#define ACN_TRACE_WAVES ACN_WALK_WAVES
#endif
#ifndef ACN_HPATH_WAVES
#define ACN_HPATH_WAVES ACN_WALK_WAVES
#endif
#ifndef ACN_WALK_MAX_STEPS
#define ACN_WALK_MAX_STEPS ( 1u << 20 )   /* safety bound of a wave's step loop (64 M rays per wave) */
#endif
#endif /* ACN_KERNEL_PARAMS_H */
