/* k_walk< true, *, true > (instrumented, with prune programs / in-line simple compounds): see acn_launch.h */
#include <hip/hip_runtime.h>
#include "acn_k_walk.h"

void acn_launch_walk_count_prune( KernelFlags f, const LevelQ& q, const WalkLaunch& w, hipStream_t stream, const SceneArgs& s )
{
    acn_variant( f.lds_nodes, [ & ]( auto L ) { ACN_LW_( true, L.value, true ); } );
}
