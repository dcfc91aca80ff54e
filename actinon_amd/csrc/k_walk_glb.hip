/* k_walk< false, false, * > (node array read from global memory / L2): see acn_launch.h */
#include <hip/hip_runtime.h>
#include "acn_k_walk.h"

void acn_launch_walk_glb( KernelFlags f, const LevelQ& q, const WalkLaunch& w, hipStream_t stream, const SceneArgs& s )
{
    acn_variant( f.prune, [ & ]( auto P ) { ACN_LW_( false, false, P.value ); } );
}
