/* k_hard_path< ... >: see acn_launch.h */
#include <hip/hip_runtime.h>
#include "acn_k_hard.h"

void acn_launch_hard_path( KernelFlags f, const LevelQ& q, size_t lds_bytes, hipStream_t stream, const SceneArgs& s,
                           unsigned long long* accum, unsigned long long* counters )
{
    acn_variant( f.count, f.prune, f.lds_nodes, [ & ]( auto C, auto P, auto L ) {
        hipLaunchKernelGGL( ( k_hard_path< C.value, L.value, P.value > ), dim3( q.grid ), dim3( 256 ), lds_bytes, stream,
            ACN_SCENE_ARGS_OF( s ), ( const HardPath* )q.hard_path, q.hard_cap, q.fetch_hard, q.children, q.child_cap, q.counts, accum, counters ); } );
}
