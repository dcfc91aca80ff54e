/* k_walk< true, *, false > (instrumented) and k_shade_hits: see acn_launch.h */
#include <hip/hip_runtime.h>
#include "acn_k_walk.h"

void acn_launch_walk_count( KernelFlags f, const LevelQ& q, const WalkLaunch& w, hipStream_t stream, const SceneArgs& s )
{
    if( f.prune ) acn_launch_walk_count_prune( f, q, w, stream, s );
    else          acn_variant( f.lds_nodes, [ & ]( auto L ) { ACN_LW_( true, L.value, false ); } );
}

void acn_launch_shade_hits( bool count, const LevelQ& q, hipStream_t stream, const SceneArgs& s,
                            unsigned long long* accum, unsigned long long* counters )
{
    acn_variant( count, [ & ]( auto C ) {
        hipLaunchKernelGGL( ( k_shade_hits< C.value > ), dim3( q.grid ), dim3( 256 ), 0, stream, ACN_SCENE_ARGS_OF( s ), ACN_TASKQ_ARGS_OF( q ),
            ( const HitRec* )q.children, q.prev_children, q.child_cap, q.fetch_hard, q.rays[ 0 ], q.ray_cap, accum, counters ); } );
}
