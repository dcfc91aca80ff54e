/* k_query.hip -- test seam: the traversal shortcuts of acn_device.h, one ray at a time (acn_query_rays, include/actinon_hip.h).
 *
 * Every op calls the device function the pipeline calls, in the arrangement of the pipeline's machine kernels (k_hard_shadow,
 * k_hard_path): 256-lane workgroups, the handle's SceneArgs, the node array staged in LDS or read from global memory, the CSG
 * stacks in LDS behind it, the plain scene (DevSceneT) or the one with interval-prune programs and in-line simple compounds
 * (DevScenePT).  Ray i runs on lane i % 64 of wave i / 64, so the caller decides which rays share a wave.  The production
 * kernels are untouched: this unit only instantiates the same templates once more. */
#include <hip/hip_runtime.h>
#include "acn_handle.h"
#include "acn_kernel_params.h"
#include "acn_variant.h"

/* results per ray: ACN_Q_STRIDE doubles; integers are stored as doubles, skip masks as their 64 raw bits */
#define ACN_Q_STRIDE ACN_QUERY_STRIDE

template< class SC >
__device__ void query_one( const SC& scv, int op, int32_t node, V3 rp, V3 rd, double limit, uint64_t skip, uint32_t pos_base, double* o )
{
    Cnt< false > cnt_;
    Cnt< false >* cnt = &cnt_;   /* what the leaf routines' macros append */
    auto n = &scv.nodes[ node ];
    const int type = n->type;
    const double nan = __builtin_nan( "" );
    if( op == ACN_Q_HIT_LANE || op == ACN_Q_HIT_UNI || op == ACN_Q_ELEMENT_HIT )
    {
        if( type == ACN_COMPOUND && op != ACN_Q_ELEMENT_HIT ) { o[ 0 ] = nan; return; }
        V3 nor = mk( 0, 0, 0 );
        int ho = -1;
        double a;
        if( op == ACN_Q_HIT_LANE )     a = obj_ray_hit_dev( sref( scv ), node, rp, rd, true, &nor, cnt );
        else if( op == ACN_Q_HIT_UNI ) a = obj_ray_hit_uni< true, SC::park >( sref( scv ), node, rp, rd, &nor, cnt );
        else                           a = element_hit< true >( scv, node, rp, rd, &nor, &ho, -F3_INF, cnt );
        o[ 0 ] = a; o[ 1 ] = nor.x; o[ 2 ] = nor.y; o[ 3 ] = nor.z; o[ 4 ] = ( double )ho;
    }
    else if( op == ACN_Q_SIDE_LANE || op == ACN_Q_SIDE_UNI )
    {
        if( type == ACN_COMPOUND ) { o[ 0 ] = nan; return; }
        o[ 0 ] = ( double )( op == ACN_Q_SIDE_LANE ? obj_side_dev( sref( scv ), node, rp, cnt ) : obj_side_uni( sref( scv ), node, true, rp, cnt ) );
    }
    else if( op == ACN_Q_PRUNE )
    {
        /* element_hit's pre-tests of a CSG root element (distance objects are never pruned) */
        const bool so = type != ACN_DISTANCE && surely_outside< ACN_PRUNE_DEPTH >( scv, node, rp, rd );
        const bool pl = type != ACN_DISTANCE && prune_run( scv, node, rp, rd, limit );
        const bool pi = type != ACN_DISTANCE && prune_run( scv, node, rp, rd, F3_INF );
        o[ 0 ] = so; o[ 1 ] = pl; o[ 2 ] = pi;
        o[ 3 ] = SC::prune && scv.elems[ scv.prune_base + ( uint32_t )node ] >= 0;   /* the node has a program */
    }
    else if( op == ACN_Q_LEAF_IV )
    {
        Iv iv; iv.lo = nan; iv.hi = nan;
        if( type == ACN_SPHERE )        iv = iv_ball( ld3( n->pos ), n->prm[ 0 ], rp, rd );
        else if( type == ACN_SQUAROID ) iv = iv_squaroid( n, rp, rd );
        else if( type == ACN_PLANE )    iv = iv_halfspace( ld3( n->pos ), ld3( n->rax + 6 ), rp, rd, false );
        o[ 0 ] = iv.lo; o[ 1 ] = iv.hi;
        if( node_has_env( n ) ) { Iv e = iv_ball( ld3( n->env_pos ), n->env_radius, rp, rd ); o[ 2 ] = e.lo; o[ 3 ] = e.hi; }
        else { o[ 2 ] = nan; o[ 3 ] = nan; }
    }
    else if( op == ACN_Q_TRANS )
    {
        if( type != ACN_COMPOUND ) { o[ 0 ] = nan; return; }
        Trans t; t.exit_nor = mk( 0, 0, 0 ); t.exit_obj = -1; t.enter_obj = -1;
        double a = root_trans_hit( scv, node, rp, rd, &t, cnt );
        o[ 0 ] = a; o[ 1 ] = t.exit_nor.x; o[ 2 ] = t.exit_nor.y; o[ 3 ] = t.exit_nor.z; o[ 4 ] = t.exit_obj; o[ 5 ] = t.enter_obj;
        /* k_shade's form, and where it says hard k_hard_path's: the fold resumed over the candidates of the in-line pass */
        Trans f; f.exit_nor = mk( 0, 0, 0 ); f.exit_obj = -1; f.enter_obj = -1;
        bool hard = false;
        uint32_t machines = 0, inline_hits = 0;
        double b = root_trans_hit_fast( scv, node, rp, rd, &f, &hard, &machines, &inline_hits, cnt );
        if( hard ) { f.exit_nor = mk( 0, 0, 0 ); f.exit_obj = -1; f.enter_obj = -1; b = root_trans_hit_rec< true >( scv, node, rp, rd, &f, resume_record( machines | inline_hits ), cnt ); }
        o[ 6 ] = b; o[ 7 ] = f.exit_nor.x; o[ 8 ] = f.exit_nor.y; o[ 9 ] = f.exit_nor.z; o[ 10 ] = f.exit_obj; o[ 11 ] = f.enter_obj; o[ 12 ] = hard;
        o[ 13 ] = ( double )( machines | inline_hits );
    }
    else if( op == ACN_Q_OCCLUDED )
    {
        if( type != ACN_COMPOUND ) { o[ 0 ] = nan; return; }
        o[ 0 ] = root_occluded( scv, node, rp, rd, limit, cnt );
        uint32_t cand = 0;
        const int fast = root_occluded_fast( scv, node, rp, rd, limit, skip, &cand, cnt );
        o[ 1 ] = fast;
        /* k_hard_shadow's form for what the in-line pass leaves undecided: resumed over its candidates */
        o[ 2 ] = nan;
        if( fast == 2 ) o[ 2 ] = root_occluded_rec< true >( scv, node, rp, rd, limit, resume_record( cand ), pos_base, cnt );
        o[ 3 ] = ( double )cand;
    }
    else if( op == ACN_Q_CONE_CULL )
    {
        /* k_shade's direct-light loop (acn_k_shade.h): node is the light, the ray origin the shading point */
        V3 fov_d; double cos_rs;
        obj_fov_dev( n, rp, &fov_d, &cos_rs );
        const M3 src_frame = m_con_z( fov_d );
        const double cyl_hgt = 1 - cos_rs;
        const uint64_t s = root_cone_cull( scv, scv.matter_root, rp, src_frame.z, 1.0 - cyl_hgt );
        ( ( uint64_t* )o )[ 0 ] = s;
        o[ 1 ] = src_frame.z.x; o[ 2 ] = src_frame.z.y; o[ 3 ] = src_frame.z.z; o[ 4 ] = 1.0 - cyl_hgt; o[ 5 ] = cyl_hgt;
    }
    else if( op == ACN_Q_SC_HIT )
    {
        if( type != ACN_COMPOUND || !( n->flags & ACN_GFLAG_SIMPLE_COMPOUND ) ) { o[ 0 ] = nan; return; }
        V3 nor = mk( 0, 0, 0 );
        int ho = -1;
        double a = F3_INF;
        if( !node_has_env( n ) || env_ray_hits( n, rp, rd, cnt ) ) a = simple_compound_hit< true >( scv, node, rp, rd, &nor, &ho, -F3_INF, cnt );
        o[ 0 ] = a; o[ 1 ] = nor.x; o[ 2 ] = nor.y; o[ 3 ] = nor.z; o[ 4 ] = ho;
        /* the any-hit form (root_occluded_fast) */
        int ho2 = -1;
        double b = F3_INF;
        if( !node_has_env( n ) || env_ray_hits( n, rp, rd, cnt ) ) b = simple_compound_hit< false >( scv, node, rp, rd, nullptr, &ho2, limit, cnt );
        o[ 5 ] = b <= limit;
    }
}

template< bool LDS, bool PRUNE >
__global__ __launch_bounds__( 256 )
void k_query( ACN_SCENE_PARAMS, int op, int32_t node, const double* __restrict__ rays, const double* __restrict__ limits, size_t n,
              uint32_t pos_base, double* __restrict__ out )
{
    ACN_SCENE_VIEW
    if( sc_in.lds_stack != ACN_NO_LDS_STACK ) sc.lds_stack = LDS ? sc.n_nodes * ( uint32_t )sizeof( GNode ) : 0u;
    if constexpr( LDS ) ACN_STAGE_NODES( sc )
    const size_t i = ( size_t )blockIdx.x * blockDim.x + threadIdx.x;
    if( i >= n ) return;
    const V3 rp = mk( rays[ 6 * i ], rays[ 6 * i + 1 ], rays[ 6 * i + 2 ] ), rd = mk( rays[ 6 * i + 3 ], rays[ 6 * i + 4 ], rays[ 6 * i + 5 ] );
    const double limit = limits ? limits[ 2 * i ] : F3_INF;
    const uint64_t skip = limits ? ( ( const uint64_t* )limits )[ 2 * i + 1 ] : 0ull;
    double* o = out + ACN_Q_STRIDE * i;
    for( int k = 0; k < ACN_Q_STRIDE; k++ ) o[ k ] = 0;
    query_one( machine_view< PRUNE, LDS >( sc ), op, node, rp, rd, limit, skip, pos_base, o );
}

/* the elements of compound `node` with the device-only bits of their headers; one lane */
__global__ void k_query_elements( ACN_SCENE_PARAMS, int32_t node, double* __restrict__ out, size_t n )
{
    ACN_SCENE_VIEW
    auto c = &sc.nodes[ node ];
    if( c->type != ACN_COMPOUND ) { out[ 0 ] = __builtin_nan( "" ); return; }
    for( int k = 0; k < c->child1 && ( size_t )k < n; k++ )
    {
        const int e = sc.elems[ c->child0 + k ];
        auto g = &sc.nodes[ e ];
        uint32_t w = 0;
        if( is_fast_type( g->type ) )                 w |= ACN_Q_EL_FAST;
        if( g->flags & ACN_GFLAG_LEAF_PAIR )          w |= ACN_Q_EL_LEAF_PAIR;
        if( g->flags & ACN_GFLAG_SIMPLE_COMPOUND )    w |= ACN_Q_EL_SIMPLE_COMPOUND;
        if( sc.elems[ sc.prune_base + ( uint32_t )e ] >= 0 ) w |= ACN_Q_EL_PROGRAM;
        if( node_has_env( g ) )                       w |= ACN_Q_EL_ENVELOPE;
        out[ ACN_Q_STRIDE * k ] = e;
        out[ ACN_Q_STRIDE * k + 1 ] = w;
        out[ ACN_Q_STRIDE * k + 2 ] = g->type;
    }
}

extern "C" int acn_query_rays( acn_scene_handle* h, int op, int32_t node, const double* rays, size_t n, const double* limits,
                               void* out )
{
    const uint32_t flags = ( uint32_t )op & ~0xFFu;
    op &= 0xFF;
    Call c( nullptr );
    if( !h ) return fail( ACN_ERR_ARG, "null argument" );
    int st = call_begin( h, &c );
    if( st != ACN_OK ) return st;
    const SceneArgs s = scene_args( h->dev, h->scene );
    if( !out || node < 0 || ( uint32_t )node >= s.dev.n_nodes || op < 0 || op >= ACN_Q_N ) return fail( ACN_ERR_ARG, "acn_query_rays: bad argument" );
    if( op != ACN_Q_ELEMENTS && n && !rays ) return fail( ACN_ERR_ARG, "acn_query_rays: no rays" );
    const bool lds = !( flags & ACN_QUERY_GLOBAL_NODES ) && h->scene.lds_bytes != 0;
    const bool prune = !( flags & ACN_QUERY_PLAIN_SCENE );
    const size_t nr = op == ACN_Q_ELEMENTS ? 0 : n;
    const size_t out_bytes = sizeof( double ) * ACN_Q_STRIDE * ( n ? n : 1 );
    DevCopies dc;
    double* d_out = ( double* )dc.make( nullptr, out_bytes );
    const double* d_rays = nr ? ( const double* )dc.make( rays, sizeof( double ) * 6 * nr ) : nullptr;
    const double* d_lim = nr && limits ? ( const double* )dc.make( limits, sizeof( double ) * 2 * nr ) : nullptr;
    if( !d_out || ( nr && !d_rays ) || ( nr && limits && !d_lim ) ) return fail( ACN_ERR_DEVICE, "device buffers of a host call" );
    HIP_TRY( hipMemsetAsync( d_out, 0, out_bytes, c.stream ) );
    if( op == ACN_Q_ELEMENTS ) hipLaunchKernelGGL( k_query_elements, dim3( 1 ), dim3( 1 ), 0, c.stream, ACN_SCENE_ARGS_OF( s ), node, d_out, n );
    else if( nr )
    {
        const dim3 grid( ( unsigned )( ( nr + 255 ) / 256 ) );
        const size_t lds_total = ( lds ? h->scene.lds_bytes : 0 ) + h->scene.lds_stack_bytes;
        acn_variant( lds, prune, [ & ]( auto L, auto P ) {
            hipLaunchKernelGGL( ( k_query< L.value, P.value > ), grid, dim3( 256 ), lds_total, c.stream, ACN_SCENE_ARGS_OF( s ), op, node, d_rays, d_lim, nr, s.elem_pos_base, d_out ); } );
    }
    HIP_TRY( hipGetLastError() );
    if( ( st = call_end( c ) ) != ACN_OK ) return st;
    if( n && ( st = DevCopies::fetch( out, d_out, out_bytes ) ) != ACN_OK ) return st;   /* out holds n rows: none for n == 0 */
    if( op == ACN_Q_ELEMENTS && n ) ( ( double* )out )[ 3 ] = ( double )h->scene.lds_bytes;   /* 0: nodes are never staged */
    return ACN_OK;
}
