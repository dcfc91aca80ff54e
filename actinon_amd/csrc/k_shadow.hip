/* k_shadow.hip -- shadow records and the history guard built on them (acn_shadow_records*, acn_shadow_limit_history*;
 * include/actinon_hip.h states both to the bit, tests/shadow_model.py restates them from the oracle's tap and in numpy).
 *
 *   k_shadow   how much of each light a surface point sees: the direct-light loop of scene_s_lum (src/scene.c:542-581, k_shade in
 *              acn_k_shade.h) with everything but the occlusion answer left out.  The arrangement is k_surface's: 256-lane workgroups,
 *              the handle's SceneArgs, the node array staged in LDS or read from global memory, the CSG stacks in LDS behind it, the
 *              production scene view.  No queue, no workspace, no atomic.
 *              LANES ARE SAMPLES.  S consecutive lanes share a position and 64 / S positions share a wave: lane t of the launch is
 *              sample t % S of position t / S.  A group's rays leave one origin inside one cone, so the root traversal stays as
 *              coherent as k_shade's.  The light loop is wave-uniform; a wave none of whose groups is SAMPLED skips it under one ballot.
 *              COUNTS ARE BALLOTS.  asked and clear of a group are the population counts of the group's slice of two ballots:
 *              integers, exact, independent of order; no shuffle, no LDS, no floating-point sum.  The per-light counts live in ten
 *              named registers picked by selects on the wave-uniform light index (an array indexed at run time would go to scratch).
 *              The occlusion answer is root_occluded outright: the cost-ordered root loop that ends when every lane is occluded.
 *              root_occluded_fast behind root_cone_cull with the resumed pass of k_hard_shadow gives the same answers
 *              (tests/test_gpu_resume_queries.py) and was measured beside it: 3.09 against 2.43 ms for 1920 x 1080 wine-glass
 *              records at S = 16 (profiles/r24/NOTES.md).  k_shade earns the cull back over a task's dozens of sample rounds; here a
 *              lane draws ONE sample per light, so the cull costs every lane what it saves it.
 *   k_shadow_limit_history   one position per lane, no scene access: the pieces of two shadow records the rule reads, one
 *              statistics record in place.  A lane whose record stays untouched writes nothing of it. */
#include <hip/hip_runtime.h>
#include "acn_launch.h"
#include "acn_kernel_params.h"
#include "acn_variant.h"
#include "acn_stats_dev.h"

#define SHADOW_PIECES ( ACN_SHADOW_STRIDE / 2 )
#define SURF_PIECES   ( ACN_SURF_STRIDE / 2 )
#define STATS_PIECES  ( ACN_STATS_STRIDE / 2 )

/* surf: [ n ][ ACN_SURF_STRIDE ], of which a lane reads pieces 0 .. 3 and 6; out: [ n ][ ACN_SHADOW_STRIDE ], written whole by the
 * first lane of the position's group: eight 16-byte stores to one 128-byte line.  log2_s: S = 1 << log2_s <= 64.
 * The grid covers n << log2_s lanes; a workgroup holds 256 >> log2_s whole positions. */
template< bool LDS, bool LEAF_LIGHTS >
__global__ __launch_bounds__( 256, ACN_TRACE_WAVES )
void k_shadow( ACN_SCENE_PARAMS, const double2* __restrict__ surf, size_t n, uint32_t log2_s, double2* __restrict__ out )
{
    ACN_SCENE_VIEW
    if( sc_in.lds_stack != ACN_NO_LDS_STACK ) sc.lds_stack = LDS ? sc.n_nodes * ( uint32_t )sizeof( GNode ) : 0u;   /* the CSG stacks follow the staged nodes */
    if constexpr( LDS ) ACN_STAGE_NODES( sc )
    const auto scv = machine_view< true, LDS >( sc );
    Cnt< false > cnt_;
    Cnt< false >* cnt = &cnt_;
    const uint32_t S = 1u << log2_s;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t sub = lane & ( S - 1u );
    const uint32_t group_first = lane & ~( S - 1u );                     /* the group's slice of a ballot: S bits from here */
    const uint64_t group_mask = S == 64u ? ~0ull : ( 1ull << S ) - 1ull;
    const size_t i = ( ( size_t )blockIdx.x * blockDim.x + threadIdx.x ) >> log2_s;
    const bool mine = i < n;

    V3 P = mk( 0, 0, 0 ), D = mk( 0, 0, 1 );
    bool sampled = false;
    if( mine )
    {
        const double2* r = surf + i * SURF_PIECES;
        const double2 s0 = r[ 0 ], s1 = r[ 1 ], s2 = r[ 2 ], s3 = r[ 3 ], s6 = r[ 6 ];
        P = mk( s0.y, s1.x, s1.y );
        D = v_neg( mk( s2.x, s2.y, s3.x ) );
        sampled = s0.x < F3_INF && !( ( uint32_t )( int32_t )s6.x & ACN_SURF_EMITTER );
    }
    const uint64_t rv0 = v_random_seed( P, 3294479285ull ) + v_random_seed( D, 3247146734ull );   /* scene.c:537 */

    NodeP lights = &sc.nodes[ sc.light_root ];
    const int n_lights = lights->child1;
    uint32_t asked_all = 0, clear_all = 0;
    uint32_t a0 = 0, a1 = 0, a2 = 0, a3 = 0, a4 = 0, c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0;
    if( __ballot( sampled ) != 0ull )
    {
        #pragma unroll 1
        for( int li = 0; li < n_lights; li++ )
        {
            const int light_idx = __builtin_amdgcn_readfirstlane( sc.elems[ lights->child0 + li ] );
            bool asked = false;
            V3 out_d = mk( 0, 0, 1 );
            double a = F3_INF;
            if( sampled )
            {
                auto light_src = &scv.nodes[ light_idx ];
                V3 fov_d; double cos_rs;
                obj_fov_dev( light_src, P, &fov_d, &cos_rs );
                const M3 src_con = m_transposed( m_con_z( fov_d ) );
                const double cyl_hgt = 1 - cos_rs;
                uint64_t rv = lcg00_jump( rv0, 2ull * ( ( uint64_t )li * S + sub ) );
                const V3 cap = v_random_sphere_cap( &rv, cyl_hgt );
                out_d = m_mlv( src_con, cap );
                if( v_mlv( out_d, D ) > 0 )
                {
                    if constexpr( LEAF_LIGHTS ) a = leaf_element_hit< false >( light_src, light_src->type, P, out_d, nullptr, cnt );
                    else a = light_hit_call( scv, light_idx, P, out_d, cnt );
                    asked = a < F3_INF;
                }
            }
            bool occluded = false;
            if( asked ) occluded = root_occluded( scv, sc.matter_root, P, out_d, a, cnt );
            const uint64_t asked_wave = __ballot( asked ), clear_wave = __ballot( asked && !occluded );
            const uint32_t ga = ( uint32_t )__builtin_popcountll( ( asked_wave >> group_first ) & group_mask );
            const uint32_t gc = ( uint32_t )__builtin_popcountll( ( clear_wave >> group_first ) & group_mask );
            asked_all += ga; clear_all += gc;
            a0 += li == 0 ? ga : 0u; a1 += li == 1 ? ga : 0u; a2 += li == 2 ? ga : 0u; a3 += li == 3 ? ga : 0u; a4 += li == 4 ? ga : 0u;
            c0 += li == 0 ? gc : 0u; c1 += li == 1 ? gc : 0u; c2 += li == 2 ? gc : 0u; c3 += li == 3 ? gc : 0u; c4 += li == 4 ? gc : 0u;
        }
    }

    if( !mine || sub != 0u ) return;
    double2* o = out + i * SHADOW_PIECES;
    if( sampled )
    {
        const double asked_d = ( double )asked_all, clear_d = ( double )clear_all;
        o[ 0 ] = make_double2( 1.0, ( double )S );
        o[ 1 ] = make_double2( ( double )n_lights, asked_d );
        o[ 2 ] = make_double2( clear_d, asked_all > 0u ? clear_d / asked_d : 0.0 );
        o[ 3 ] = make_double2( ( double )c0, ( double )c1 );
        o[ 4 ] = make_double2( ( double )c2, ( double )c3 );
        o[ 5 ] = make_double2( ( double )c4, ( double )a0 );
        o[ 6 ] = make_double2( ( double )a1, ( double )a2 );
        o[ 7 ] = make_double2( ( double )a3, ( double )a4 );
    }
    else
    {
        #pragma unroll
        for( int k = 0; k < SHADOW_PIECES; k++ ) o[ k ] = make_double2( 0.0, 0.0 );
    }
}

/* lanes of one launch: a multiple of the workgroup size, far below the grid limit of 2^31 - 1 workgroups */
#define ACN_SHADOW_LAUNCH_LANES ( ( size_t )1 << 30 )

void acn_launch_shadow( bool lds_nodes, bool leaf_lights, size_t lds_bytes, hipStream_t stream, const SceneArgs& s, const double* surface,
                        size_t n, uint32_t log2_samples, double* out )
{
    const size_t per_launch = ACN_SHADOW_LAUNCH_LANES >> log2_samples;
    for( size_t first = 0; first < n; first += per_launch )
    {
        const size_t cnt = n - first < per_launch ? n - first : per_launch;
        const dim3 grid( ( unsigned )( ( ( cnt << log2_samples ) + 255 ) / 256 ) );
        const double2* in = ( const double2* )( surface + ( size_t )ACN_SURF_STRIDE * first );
        double2* o = ( double2* )( out + ( size_t )ACN_SHADOW_STRIDE * first );
        acn_variant( lds_nodes, leaf_lights, [ & ]( auto L, auto F ) {
            hipLaunchKernelGGL( ( k_shadow< L.value, F.value > ), grid, dim3( 256 ), lds_bytes, stream, ACN_SCENE_ARGS_OF( s ), in, cnt, log2_samples, o ); } );
    }
}

/* the steps of acn_shadow_limit_history* for the lane's position (include/actinon_hip.h numbers them) */
__global__ __launch_bounds__( 256 )
void k_shadow_limit_history( double2* __restrict__ stats, const double* __restrict__ motion, const double2* __restrict__ cur_shadow,
                             const double2* __restrict__ prev_shadow, size_t n, uint64_t width, uint64_t height, ShadowHistorySetup su,
                             double* __restrict__ out_change )
{
    const size_t i = ( size_t )blockIdx.x * blockDim.x + threadIdx.x;
    if( i >= n ) return;
    double change = __builtin_nan( "" );
    double2* t = stats + i * STATS_PIECES;
    const double2 t0 = t[ 0 ];
    const double qx = motion[ 2 * i ], qy = motion[ 2 * i + 1 ];
    /* 1 HISTORY */
    if( !stats_empty( t0.x ) && qx == qx && qy == qy )
    {
        /* 2 PLACE */
        const double x = __builtin_floor( qx ), y = __builtin_floor( qy );
        if( x >= 0.0 && x < ( double )width && y >= 0.0 && y < ( double )height )
        {
            const size_t at = ( size_t )y * ( size_t )width + ( size_t )x;
            const double2* c = cur_shadow + i * SHADOW_PIECES;
            const double2* p = prev_shadow + at * SHADOW_PIECES;
            const double2 ch = c[ 0 ], ph = p[ 0 ];
            /* 3 SAMPLED */
            if( ch.x == 1.0 && ph.x == 1.0 )
            {
                /* 4 CHANGE */
                const double2 c1 = c[ 1 ], c2 = c[ 2 ], c3 = c[ 3 ], c4 = c[ 4 ], c5 = c[ 5 ];
                const double2 p1 = p[ 1 ], p2 = p[ 2 ], p3 = p[ 3 ], p4 = p[ 4 ], p5 = p[ 5 ];
                const double cl[ 5 ] = { c3.x, c3.y, c4.x, c4.y, c5.x }, pl[ 5 ] = { p3.x, p3.y, p4.x, p4.y, p5.x };
                double m = 0.0;
                #pragma unroll
                for( int l = 0; l < 5; l++ )
                {
                    const double term = acn_fabs( cl[ l ] / ch.y - pl[ l ] / ph.y );
                    if( ( double )l < c1.x && term > m ) m = term;
                }
                const double term = acn_fabs( c2.x / ( ch.y * c1.x ) - p2.x / ( ph.y * p1.x ) );
                if( term > m ) m = term;
                change = m;
                /* 5 LIMIT */
                if( change > su.tolerance )
                {
                    if( su.drop )
                    {
                        #pragma unroll
                        for( int k = 0; k < STATS_PIECES; k++ ) t[ k ] = make_double2( 0.0, 0.0 );
                    }
                    else if( t0.x > su.cap )
                    {
                        const double f = su.cap / t0.x;
                        const double2 t2 = t[ 2 ], t3 = t[ 3 ];
                        t[ 0 ] = make_double2( su.cap, t0.y );
                        t[ 2 ] = make_double2( t2.x * f, t2.y * f );
                        t[ 3 ] = make_double2( t3.x * f, t3.y );
                    }
                }
            }
        }
    }
    if( out_change ) out_change[ i ] = change;
}

void acn_launch_shadow_limit_history( double* stats, const double* motion, const double* cur_shadow, const double* prev_shadow, size_t n,
                                      uint64_t width, uint64_t height, const ShadowHistorySetup& su, double* out_change, hipStream_t stream )
{
    hipLaunchKernelGGL( k_shadow_limit_history, dim3( ( unsigned )( ( n + 255 ) / 256 ) ), dim3( 256 ), 0, stream, ( double2* )stats, motion,
                        ( const double2* )cur_shadow, ( const double2* )prev_shadow, n, width, height, su, out_change );
}
