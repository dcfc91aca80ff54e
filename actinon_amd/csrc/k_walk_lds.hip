/* k_walk< false, true, * > (node array staged in LDS) and the head of the launch chain of k_walk: see acn_launch.h */
#include <hip/hip_runtime.h>
#include "acn_k_walk.h"

void acn_launch_walk( KernelFlags f, const LevelQ& q, const WalkLaunch& w, hipStream_t stream, const SceneArgs& s )
{
    if( f.count )           acn_launch_walk_count( f, q, w, stream, s );
    else if( !f.lds_nodes ) acn_launch_walk_glb( f, q, w, stream, s );
    else                    acn_variant( f.prune, [ & ]( auto P ) { ACN_LW_( false, true, P.value ); } );
}
