/* k_surface.hip -- the surface a ray meets, one record per ray (acn_surface_rays, acn_surface_positions; include/actinon_hip.h).
 *
 * The pipeline computes distance, exit normal, the two objects of the media transition and the surface colour for every ray it
 * traces and keeps only the radiance.  This unit hands them out: one ray per lane in the arrangement of the machine kernels
 * (256-lane workgroups, the handle's SceneArgs, CSG stacks in LDS, the production scene view), scene_trans_hit_dev for the hit,
 * obj_color_dev for the colour.  There is no queue, no workspace and no atomic: a lane owns its ray from the first root
 * traversal to the one 128-byte record it writes, so a surface call leaves what the render calls learned and allocated alone.
 *
 * ACN_SURF_FOLLOW walks the dominant specular branch (Fresnel reflection, chromatic reflection, refraction: the intensities
 * scene_s_lum hands its children, src/scene.c:473-653, trace_min_intensity left out) to the first diffuse or emitting surface.
 * Lanes finish at different hops; the hop loop is wave-level around ONE in-line copy of the root traversal, which therefore
 * stays wave-uniform.  The mode is a template argument: the FIRST_HIT kernel carries neither the loop nor the Fresnel code. */
#include <hip/hip_runtime.h>
#include "acn_launch.h"
#include "acn_kernel_params.h"
#include "acn_variant.h"

/* The material rules of scene_s_lum for one hit (src/scene.c:432-470), with the expressions of shade_hit (acn_queues.h):
 * what the enter object sets, then what the exit object overrides. */
struct SurfMat
{
    double trix, fresnel_reflectivity, chromatic_reflectivity, diffuse_reflectivity;
    bool emitter, transparent;
};

DEV SurfMat surface_material( const DevScene& sc, const Trans& trans )
{
    SurfMat m;
    m.trix = 1.0; m.fresnel_reflectivity = 0; m.chromatic_reflectivity = 0; m.diffuse_reflectivity = 0;
    m.emitter = false; m.transparent = false;
    MatP enter_obj = trans.enter_obj >= 0 ? &sc.mats[ trans.enter_obj ] : nullptr;
    MatP exit_obj  = trans.exit_obj  >= 0 ? &sc.mats[ trans.exit_obj  ] : nullptr;
    if( enter_obj && enter_obj->radiance > 0 ) m.emitter = true;   /* :432-437: scene_s_lum returns here */
    if( enter_obj )   /* :448-462 */
    {
        m.trix = enter_obj->refractive_index;
        m.fresnel_reflectivity   = ( enter_obj->fresnel_reflectivity != 0 && enter_obj->refractive_index != 1.0 ) ? 1.0 : 0.0;
        m.chromatic_reflectivity = enter_obj->chromatic_reflectivity;
        m.diffuse_reflectivity   = enter_obj->diffuse_reflectivity;
        m.transparent            = v_sqr( ld3( enter_obj->transparency ) ) > 0;
    }
    if( exit_obj )   /* :464-470 */
    {
        m.trix /= exit_obj->refractive_index;
        m.fresnel_reflectivity = 1.0;
        m.diffuse_reflectivity = m.chromatic_reflectivity = 0;
        m.transparent = true;
    }
    return m;
}

DEV uint32_t surface_kind( const DevScene& sc, const SurfMat& m, const Trans& trans, bool light_root )
{
    uint32_t k = 0;
    if( m.emitter )                     k |= ACN_SURF_EMITTER;
    if( m.diffuse_reflectivity > 0 )    k |= ACN_SURF_DIFFUSE;
    if( m.chromatic_reflectivity > 0 )  k |= ACN_SURF_CHROMATIC;
    if( m.fresnel_reflectivity > 0 )    k |= ACN_SURF_FRESNEL;
    if( m.transparent )                 k |= ACN_SURF_TRANSPARENT;
    if( light_root )                    k |= ACN_SURF_LIGHT_ROOT;
    return k;
}

/* scene_s_trans_hit (src/scene.c:362-382) with the root that won: lights first, matter only if strictly nearer.  The one
 * in-line copy of the root traversal of scene_trans_hit_dev, plus the bit the record reports. */
template< class SC >
DEV double surface_trans_hit( const SC& scv, V3 rp, V3 rd, Trans* trans, bool* light_root )
{
    Cnt< false > cnt_;
    Cnt< false >* cnt = &cnt_;
    double min_a = F3_INF;
    double a;
    Trans trans_l;
    trans_l.exit_nor = mk( 0, 0, 0 ); trans_l.exit_obj = -1; trans_l.enter_obj = -1;
    #pragma unroll 1
    for( int k = 0; k < 2; k++ )
    {
        if( ( a = root_trans_hit( scv, k ? scv.matter_root : scv.light_root, rp, rd, &trans_l, cnt ) ) < min_a )
        {
            min_a = a;
            *trans = trans_l;
            *light_root = k == 0;
        }
    }
    return min_a;
}

/* rays != nullptr: [ n ][ 6 ] origin, direction; else pos_xy: [ n ][ 2 ] sample positions, through camera_ray.
 * out: [ n ][ ACN_SURF_STRIDE ], written whole by the ray's lane: eight 16-byte stores to one 128-byte line. */
template< int MODE, bool LDS >
__global__ __launch_bounds__( 256, ACN_TRACE_WAVES )
void k_surface( ACN_SCENE_PARAMS, const double* __restrict__ rays, const double* __restrict__ pos_xy, size_t n, double* __restrict__ out )
{
    ACN_SCENE_VIEW
    if( sc_in.lds_stack != ACN_NO_LDS_STACK ) sc.lds_stack = LDS ? sc.n_nodes * ( uint32_t )sizeof( GNode ) : 0u;   /* the CSG stacks follow the staged nodes */
    if constexpr( LDS ) ACN_STAGE_NODES( sc )
    const size_t i = ( size_t )blockIdx.x * blockDim.x + threadIdx.x;
    const bool mine = i < n;
    V3 rp = mk( 0, 0, 0 ), rd = mk( 0, 0, 1 );
    if( mine )
    {
        if( rays ) { rp = ld3( rays + 6 * i ); rd = ld3( rays + 6 * i + 3 ); }
        else camera_ray( sc, pos_xy[ 2 * i ], pos_xy[ 2 * i + 1 ], &rp, &rd );
        rd = v_of_length( rd, 1.0 );   /* vectors.h:148-154, as k_seed_rays: a camera ray stays as it is, bit for bit */
    }

    Trans trans;
    trans.exit_nor = mk( 0, 0, 0 ); trans.exit_obj = -1; trans.enter_obj = -1;
    double dist = 0.0, a = F3_INF, weight = 1.0;
    uint32_t kind = 0, hops = 0;
    bool light_root = false;

    if constexpr( MODE == ACN_SURF_FIRST_HIT )
    {
        if( mine ) a = surface_trans_hit( machine_view< true, LDS >( sc ), rp, rd, &trans, &light_root );
        dist = a;
        if( a < F3_INF ) kind = surface_kind( sc, surface_material( sc, trans ), trans, light_root );
    }
    else
    {
        const uint32_t max_hits = sc.prm.trace_depth > 1 ? ( uint32_t )sc.prm.trace_depth : 1u;
        bool live = mine;
        #pragma unroll 1
        while( __ballot( live ) )
        {
            if( live )
            {
                trans.exit_nor = mk( 0, 0, 0 ); trans.exit_obj = -1; trans.enter_obj = -1;
                a = surface_trans_hit( machine_view< true, LDS >( sc ), rp, rd, &trans, &light_root );
                dist += a;
                live = a < F3_INF;
            }
            if( live )
            {
                const SurfMat m = surface_material( sc, trans );
                kind = surface_kind( sc, m, trans, light_root );
                /* the shares scene_s_lum hands on, in its order: Fresnel reflection :475-477, chromatic reflection :500-502,
                 * the diffuse block :526-629, refraction :633-637 */
                V3 refl_d = rd;
                double refl = 0;
                if( !m.emitter && m.fresnel_reflectivity > 0 ) refl = fresnel_reflection( rd, trans.exit_nor, m.trix, &refl_d ) * m.fresnel_reflectivity;
                double rest = 1.0 - refl;
                const double w0 = refl;
                const double w1 = m.chromatic_reflectivity * rest; rest = rest * ( 1.0 - m.chromatic_reflectivity );
                const double w2 = m.diffuse_reflectivity * rest;   rest = rest * ( 1.0 - m.diffuse_reflectivity );
                const double w3 = m.transparent ? rest : 0.0;
                int best = 0; double bw = w0;
                if( w1 > bw ) { best = 1; bw = w1; }
                if( w2 > bw ) { best = 2; bw = w2; }
                if( w3 > bw ) { best = 3; bw = w3; }
                const bool go = !m.emitter && bw > 0 && best != 2;
                if( go && hops + 1u >= max_hits ) kind |= ACN_SURF_CUT;
                live = go && !( kind & ACN_SURF_CUT );
                if( live )
                {
                    V3 nd = refl_d;
                    if( best == 1 ) nd = v_reflection( rd, trans.exit_nor );
                    if( best == 3 ) nd = fresnel_refraction( rd, trans.exit_nor, m.trix );
                    rp = ray_pos( rp, rd, best == 3 ? a + 2.0 * F3_EPS : a );
                    rd = nd;
                    weight *= bw;
                    hops++;
                }
            }
        }
    }

    if( !mine ) return;
    double2* o = ( double2* )( out + ( size_t )ACN_SURF_STRIDE * i );
    if( a < F3_INF )
    {
        const V3 pos = ray_pos( rp, rd, a );   /* as shade_hit forms pos */
        const V3 col = obj_color_dev( sc, trans.enter_obj >= 0 ? trans.enter_obj : trans.exit_obj, pos );
        o[ 0 ] = make_double2( dist, pos.x );
        o[ 1 ] = make_double2( pos.y, pos.z );
        o[ 2 ] = make_double2( trans.exit_nor.x, trans.exit_nor.y );
        o[ 3 ] = make_double2( trans.exit_nor.z, ( double )trans.enter_obj );
        o[ 4 ] = make_double2( ( double )trans.exit_obj, col.x );
        o[ 5 ] = make_double2( col.y, col.z );
        o[ 6 ] = make_double2( ( double )kind, ( double )hops );
        o[ 7 ] = make_double2( weight, 0.0 );
    }
    else
    {
        o[ 0 ] = make_double2( F3_INF, 0.0 );
        o[ 1 ] = make_double2( 0.0, 0.0 );
        o[ 2 ] = make_double2( 0.0, 0.0 );
        o[ 3 ] = make_double2( 0.0, -1.0 );
        o[ 4 ] = make_double2( -1.0, 0.0 );
        o[ 5 ] = make_double2( 0.0, 0.0 );
        o[ 6 ] = make_double2( 0.0, ( double )hops );
        o[ 7 ] = make_double2( weight, 0.0 );
    }
}

/* rays of one launch: a multiple of the workgroup size, far below the grid limit of 2^31 - 1 workgroups */
#define ACN_SURF_LAUNCH_RAYS ( ( size_t )1 << 30 )

void acn_launch_surface( uint32_t mode, bool lds_nodes, size_t lds_bytes, hipStream_t stream, const SceneArgs& s,
                         const double* rays, const double* pos_xy, size_t n, double* out )
{
    for( size_t first = 0; first < n; first += ACN_SURF_LAUNCH_RAYS )
    {
        const size_t cnt = n - first < ACN_SURF_LAUNCH_RAYS ? n - first : ACN_SURF_LAUNCH_RAYS;
        const dim3 grid( ( unsigned )( ( cnt + 255 ) / 256 ) );
        const double* r = rays ? rays + 6 * first : nullptr;
        const double* p = pos_xy ? pos_xy + 2 * first : nullptr;
        double* o = out + ( size_t )ACN_SURF_STRIDE * first;
        acn_variant( mode == ACN_SURF_FOLLOW, lds_nodes, [ & ]( auto F, auto L ) {
            hipLaunchKernelGGL( ( k_surface< F.value ? ACN_SURF_FOLLOW : ACN_SURF_FIRST_HIT, L.value > ), grid, dim3( 256 ), lds_bytes, stream, ACN_SCENE_ARGS_OF( s ), r, p, cnt, o ); } );
    }
}
