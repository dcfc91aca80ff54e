/* acn_dev_leaves.h -- what a ray or a point meets at one node: plane, sphere, squaroid and distance object (hit and side), Fresnel,
 * node access, envelopes, the roughness perturbation, and the leaf pairs with their operands. */
#ifndef ACN_DEV_LEAVES_H
#define ACN_DEV_LEAVES_H

#include "acn_dev_base.h"
#include "acn_dev_scene.h"
#include "acn_costs.h"

#pragma clang fp contract(off)

/* ---- gmath.h:38-97 ---- */
template< class CT > DEV double plane_ray_hit( V3 pos, V3 nor, V3 rp, V3 rd, bool want_nor, V3* p_nor, CT* cnt )
{
    cnt->cost( ACN_F_PLANE_HIT );
    double div = v_mlv( nor, rd );
    if( div == 0 ) return F3_INF;
    double offs = v_sub_mlv( pos, rp, nor ) / div;
    if( want_nor ) *p_nor = nor;
    return ( offs > 0 ) ? offs - F3_EPS : F3_INF;
}

template< class CT > DEV double sphere_ray_hit( V3 pos, double r, V3 rp, V3 rd, bool want_nor, V3* p_nor, CT* cnt )
{
    V3 p = v_sub( rp, pos );
    double s = v_mlv( p, rd );
    double q = v_sqr( p ) - ( r * r );
    double s2 = s * s;
    if( s2 < q ) { cnt->cost( ACN_F_SPHERE_MISS ); return F3_INF; }
    double offs = F3_INF;
    if( s < 0 && q > 0 )
    {
        offs = -s - acn_sqrt( s2 - q ) - F3_EPS;
    }
    else if( s < 0 || q < 0 )
    {
        offs = -s + acn_sqrt( s2 - q ) - F3_EPS;
    }
    if( offs < F3_INF && want_nor ) *p_nor = v_of_length( v_sub( ray_pos( rp, rd, offs ), pos ), 1.0 );
    cnt->cost( offs < F3_INF ? ( want_nor ? ACN_F_SPHERE_HIT_NOR : ACN_F_SPHERE_HIT ) : ACN_F_SPHERE_MISS );
    return offs;
}

template< class CT > DEV int sphere_observer_side( V3 pos, double r, V3 observer, CT* cnt )
{
    cnt->cost( ACN_F_SIDE_SPHERE );
    V3 diff = v_sub( observer, pos );
    return ( v_sqr( diff ) > r * r ) ? 1 : -1;
}

/* ---- gmath.c:68-113 ---- */
DEV double fresnel_reflection( V3 dir_i, V3 exit_nor, double trix, V3* dir )
{
    double c = v_mlv( dir_i, exit_nor );
    double f = c < 0 ? trix : 1.0 / trix;
    double cos_ai = acn_fabs( c );
    cos_ai = cos_ai > 1.0 ? 1.0 : cos_ai;
    double sin_ai = acn_sqrt( 1.0 - cos_ai * cos_ai );
    double sin_at = sin_ai * f;
    double reflectance = 1.0;
    if( sin_at < 1 )
    {
        double cos_at = acn_sqrt( 1.0 - sin_at * sin_at );
        double rs = f_sqr( ( f * cos_ai - cos_at ) / ( f * cos_ai + cos_at ) );
        double rp = f_sqr( ( f * cos_at - cos_ai ) / ( f * cos_at + cos_ai ) );
        reflectance = ( rs + rp ) * 0.5;
    }
    *dir = v_reflection( dir_i, exit_nor );
    return reflectance;
}

DEV V3 fresnel_refraction( V3 dir_i, V3 exit_nor, double trix )
{
    double c = v_mlv( dir_i, exit_nor );
    double f = c < 0 ? trix : 1.0 / trix;
    double a = f;
    double q = f * f * ( 1.0 - c * c );
    if( q < 1.0 )
    {
        double b = -f * c + ( c > 0 ? acn_sqrt( 1.0 - q ) : -acn_sqrt( 1.0 - q ) );
        return v_add( v_mlf( dir_i, a ), v_mlf( exit_nor, b ) );
    }
    return dir_i;
}

/* ---- node access ---- */
/* A node that is visited with the same index in every lane is named through this macro.  The view holds the pointer and nothing
 * else: copying the whole 192-byte record into SGPRs at once was measured twice and lost both times (DESIGN.md sections 4c, 4d).
 * It is not a pass-through for the compiler, though: with ACN_NODE as a plain `const auto name = expr;` the .text of k_surface
 * and of k_shadow changes (same notes, same .rodata; make digests), so taking the view out is a kernel change to be measured. */
template< class NP > struct NodeView { NP p; DEV NodeView( NP q ) : p( q ) {} DEV NP ptr() const { return p; } };
#define ACN_NODE( name, expr ) const auto name##_view_ = NodeView< decltype( expr ) >( expr ); const auto name = name##_view_.ptr();

template< class NP > DEV bool node_has_env( NP n ) { return ( n->flags & ACN_NODE_HAS_ENVELOPE ) != 0; }
template< class NP > DEV M3 node_rax( NP n )
{
    M3 m;
    m.x = ld3( n->rax ); m.y = ld3( n->rax + 3 ); m.z = ld3( n->rax + 6 );
    return m;
}
/* envelope_s_ray_hits (objects.c:90-93) = sphere_ray_hit( ... ) < f3_inf.  Only the predicate is needed: by
 * gmath.h:64-83 the offset is finite exactly when s*s >= q and ( s < 0 or q < 0 ) -- the square root of the
 * non-negative discriminant is finite for finite inputs -- so the sqrt is not evaluated. */
template< class NP, class CT > DEV bool env_ray_hits( NP n, V3 rp, V3 rd, CT* cnt );
/* the same on an envelope given by value */
template< class CT > DEV bool env_ray_hits_raw( V3 env_pos, double r, V3 rp, V3 rd, CT* cnt )
{
    V3 p = v_sub( rp, env_pos );
    double s = v_mlv( p, rd );
    double q = v_sqr( p ) - ( r * r );
    double s2 = s * s;
    bool hit = !( s2 < q ) && ( ( s < 0 && q > 0 ) || ( s < 0 || q < 0 ) );
    cnt->cost( hit ? ACN_F_ENV_HIT : ACN_F_ENV_MISS );
    return hit;
}
template< class NP, class CT > DEV bool env_ray_hits( NP n, V3 rp, V3 rd, CT* cnt )
{
    V3 p = v_sub( rp, ld3( n->env_pos ) );
    double r = n->env_radius;
    double s = v_mlv( p, rd );
    double q = v_sqr( p ) - ( r * r );
    double s2 = s * s;
    bool hit = !( s2 < q ) && ( ( s < 0 && q > 0 ) || ( s < 0 || q < 0 ) );
    cnt->cost( hit ? ACN_F_ENV_HIT : ACN_F_ENV_MISS );
    return hit;
}
template< class NP, class CT > DEV int env_side( NP n, V3 pos, CT* cnt ) { return sphere_observer_side( ld3( n->env_pos ), n->env_radius, pos, cnt ); }

/* ---- distance.c:39-42, 83-92 ---- */
template< class NP, class CT > DEV double sdf_eval( NP n, V3 pos, CT* cnt )
{
    if( n->sdf_kind == ACN_SDF_TORUS )
    {
        cnt->cost( ACN_F_SDF_TORUS );
        double x = pos.x;
        double y = pos.y;
        double f = acn_sqrt( x * x + y * y );
        double f_inv = ( f > 0 ) ? ( 1.0 / f ) : 1.0;
        x *= f_inv;
        y *= f_inv;
        return acn_sqrt( f_sqr( x - pos.x ) + f_sqr( y - pos.y ) + f_sqr( pos.z ) ) - n->prm[ 1 ];
    }
    cnt->cost( ACN_F_SDF_SPHERE );
    return acn_sqrt( f_sqr( pos.x ) + f_sqr( pos.y ) + f_sqr( pos.z ) ) - 1.0;
}

/* ---- leaves ---- */
template< class NP, class CT > DEV double squaroid_ray_hit( NP o, V3 rp, V3 rd, bool want_nor, V3* p_nor, CT* cnt )   /* objects.c:778-821 */
{
    cnt->cost( ACN_F_SQUAROID_MISS );
    M3 rax = node_rax( o );
    double oa = o->prm[ 0 ], ob = o->prm[ 1 ], oc = o->prm[ 2 ], orr = o->prm[ 3 ];
    V3 p = m_mlv( rax, v_sub( rp, ld3( o->pos ) ) );
    V3 d = m_mlv( rax, rd );
    double f  = oa * d.x * d.x + ob * d.y * d.y + oc * d.z * d.z;
    double fs = oa * d.x * p.x + ob * d.y * p.y + oc * d.z * p.z;
    double fq = oa * p.x * p.x + ob * p.y * p.y + oc * p.z * p.z + orr;
    double a = F3_INF;
    if( f != 0 )
    {
        double f_inv = 1.0 / f;
        double s = fs * f_inv;
        double q = fq * f_inv;
        double rr = s * s - q;
        if( rr < 0 ) return F3_INF;
        rr = acn_sqrt( rr );
        a = -s - rr;
        if( a < 0 ) a = -s + rr;
        if( a < 0 ) a = F3_INF;
    }
    else
    {
        a = ( fq != 0 ) ? -fs / ( 2 * fq ) : F3_INF;
    }
    if( a == F3_INF ) return F3_INF;
    cnt->cost( ( want_nor ? ACN_F_SQUAROID_HIT_NOR : ACN_F_SQUAROID_HIT ) - ACN_F_SQUAROID_MISS );
    if( want_nor )
    {
        double x = p.x + a * d.x;
        double y = p.y + a * d.y;
        double z = p.z + a * d.z;
        V3 n1 = mk( x * oa, y * ob, z * oc );
        *p_nor = v_of_length( m_tmlv( rax, n1 ), 1.0 );
    }
    return a - F3_EPS;
}

template< class NP, class CT > DEV int squaroid_side( NP o, V3 pos, CT* cnt )   /* objects.c:823-827 */
{
    cnt->cost( ACN_F_SIDE_SQUAROID );
    M3 rax = node_rax( o );
    V3 p = m_mlv( rax, v_sub( pos, ld3( o->pos ) ) );
    return ( o->prm[ 0 ] * p.x * p.x + o->prm[ 1 ] * p.y * p.y + o->prm[ 2 ] * p.z * p.z + o->prm[ 3 ] ) > 0 ? 1 : -1;
}

template< class NP, class CT >
DEVN double distance_ray_hit( NP o, V3 rp, V3 rd, bool want_nor, V3* p_nor, CT* cnt )   /* objects.c:903-959 */
{
    M3 rax = node_rax( o );
    double inv_scale = o->prm[ 0 ];
    V3 p = rp;
    double offs0 = 0;
    if( node_has_env( o ) )
    {
        if( env_side( o, rp, cnt ) == 1 )
        {
            offs0 = sphere_ray_hit( ld3( o->env_pos ), o->env_radius, rp, rd, false, nullptr, cnt );
            if( offs0 >= F3_INF ) return F3_INF;
            p = ray_pos( rp, rd, offs0 );
        }
    }
    p = v_mlf( m_mlv( rax, v_sub( p, ld3( o->pos ) ) ), inv_scale );
    V3 d = m_mlv( rax, rd );

    double offs1 = 0;
    double dist = sdf_eval( o, p, cnt );
    unsigned evals = 1;
    int cycles = o->cycles;
    if( dist > 0 )
    {
        for( int i = 0; i < cycles; i++ )
        {
            offs1 += dist + F3_EPS;
            dist = sdf_eval( o, ray_pos( p, d, offs1 ), cnt );
            evals++;
            if( dist < 0 || dist > F3_MAG ) break;
        }
    }
    else
    {
        for( int i = 0; i < cycles; i++ )
        {
            offs1 -= dist - F3_EPS;
            dist = sdf_eval( o, ray_pos( p, d, offs1 ), cnt );
            evals++;
            if( dist > 0 || dist < -F3_MAG ) break;
        }
    }
    cnt->add( CNT_SDF_EVAL, evals );
    cnt->cost( ACN_F_SDF_RAY + ACN_F_SDF_STEP * ( evals - 1 ) );
    if( f_abs( dist ) <= F3_EPS )
    {
        if( want_nor )
        {
            cnt->cost( ACN_F_SDF_NORMAL );
            V3 q = ray_pos( p, d, offs1 );
            double d0 = sdf_eval( o, q, cnt );
            V3 n;
            n.x = ( sdf_eval( o, mk( q.x + F3_EPS, q.y, q.z ), cnt ) - d0 ) / F3_EPS;
            n.y = ( sdf_eval( o, mk( q.x, q.y + F3_EPS, q.z ), cnt ) - d0 ) / F3_EPS;
            n.z = ( sdf_eval( o, mk( q.x, q.y, q.z + F3_EPS ), cnt ) - d0 ) / F3_EPS;
            *p_nor = v_of_length( m_tmlv( rax, n ), 1.0 );
        }
        return offs0 + ( offs1 / inv_scale ) - F3_EPS;
    }
    return F3_INF;
}

template< class NP, class CT > DEV int distance_side( NP o, V3 pos, CT* cnt )   /* objects.c:961-966 */
{
    cnt->cost( ACN_F_SIDE_SDF );
    if( node_has_env( o ) && env_side( o, pos, cnt ) == 1 ) return 1;
    M3 rax = node_rax( o );
    V3 p = v_mlf( m_mlv( rax, v_sub( pos, ld3( o->pos ) ) ), o->prm[ 0 ] );
    return sdf_eval( o, p, cnt ) > 0 ? 1 : -1;
}

/* objects.c:267-282.  A REAL call: the perturbation sits behind every one of the
 * ~130 places where a hit returns a normal (leaves, operands, pairs, composites), three logarithms and a seed each -- in line
 * that was 35 - 40 % of k_walk's 1.4 MB of code, in scenes of which most (the wine glass, the diamond, many_spheres) have no rough
 * surface at all: the hot code was spread over twice the instruction-cache lines it needs.  A rough surface pays a call. */
DEVN V3 roughness_apply( double surface_roughness, V3 n, V3 hit_pos )
{
    uint64_t rv = v_random_seed( hit_pos, 1246 );
    double f;
    f = f3_rnd0( &rv ) * 0.99;
    n.x += surface_roughness * acn_log( ( 1.0 - f ) / ( 1.0 + f ) );
    f = f3_rnd0( &rv ) * 0.99;
    n.y += surface_roughness * acn_log( ( 1.0 - f ) / ( 1.0 + f ) );
    f = f3_rnd0( &rv ) * 0.99;
    n.z += surface_roughness * acn_log( ( 1.0 - f ) / ( 1.0 + f ) );
    return v_of_length( n, 1.0 );
}
template< class NP, class CT > DEV V3 roughness_normal( NP hdr, V3 n, V3 hit_pos, CT* cnt )
{
    cnt->cost( ACN_F_ROUGHNESS, ACN_T_ROUGHNESS );
    return roughness_apply( hdr->surface_roughness, n, hit_pos );
}

/* ------------------------------------------------------------------------------------------------------------------ */
/* Leaf pairs.  Most composites at the bottom of a CSG tree combine two simple operands -- a plane, sphere or squaroid,
 * possibly complemented (slabs, lenses, capped cylinders; 5 of the wine glass's 9 pairs, the whole liquid).  The upload
 * step marks such pairs (ACN_GFLAG_LEAF_PAIR) and both machines evaluate them in line: the same sequence of child
 * evaluations, side tests and walk steps as the general frames (objects.c:1052-1094 / 1209-1251, 1096-1099 / 1253-1256),
 * without frame, stack or nested loops. */

template< class NP, class CT > DEV int simple_leaf_side( NP g, V3 pos, CT* cnt )
{
    int type = g->type;
    if( type == ACN_PLANE )  { cnt->cost( ACN_F_SIDE_PLANE ); return v_sub_mlv( pos, ld3( g->pos ), ld3( g->rax + 6 ) ) > 0 ? 1 : -1; }
    if( type == ACN_SPHERE ) return sphere_observer_side( ld3( g->pos ), g->prm[ 0 ], pos, cnt );
    return squaroid_side( g, pos, cnt );
}

/* Where a ray's ORIGIN lives while a CSG object is evaluated.  The machines of k_walk run at 128 VGPRs, and the value the
 * allocator gives up first is the origin of the step's ray: stored to scratch once and re-loaded at 97 places -- every leaf and
 * envelope test at a frame the ray enters unchanged (ISA of round 4, scripts/isa_scratch.py) -- ~60 % of the kernel's scratch loads
 * and most of its 22 GB per frame.  It is one value per lane for the whole evaluation of a frame, so the lock-step machine parks
 * it in LDS (three planes of 256 doubles behind the stacks and the pool) and the operand code reads it where it uses it: a
 * ds_read, ~64 cycles, no VMEM slot.  A pair's alternating walk continues from a DERIVED origin that lives for one operand
 * evaluation: a plain V3.  The operand / pair code takes either through org_get(). */
struct OrgLds
{
    volatile double ACN_LDS* p;
    DEV V3 get() const { return mk( p[ 0 ], p[ ACN_LDS_LANES ], p[ 2 * ACN_LDS_LANES ] ); }
    DEV void set( V3 v ) const { p[ 0 ] = v.x; p[ ACN_LDS_LANES ] = v.y; p[ 2 * ACN_LDS_LANES ] = v.z; }
};
DEV V3 org_get( const V3& v ) { return v; }
DEV V3 org_get( const OrgLds& o ) { return o.get(); }

/* Pairs of level L: both operands are a simple leaf, NEG( simple leaf ) or -- for L = 2 -- a level-1 pair.  The
 * functions below are the reference's obj_side / obj_ray_hit for such operands and pairs, recursion unrolled by L.
 * (Level-1 operands as real function calls instead of in-line expansion: 69.4 vs 57.4 ms on c2 -- calls spill.) */
template< int L, class SR, class NP, class CT > DEV int pair_side( SR sc, NP n, V3 pos, CT* cnt );
template< int L, bool SPLIT = false, class SR, class NP, class O, class CT > DEV double pair_hit( SR sc, NP n, O rp, V3 rd, bool want_nor, V3* nor, CT* cnt );

/* An operand that is NEG( simple leaf ) goes through the SAME copy of the leaf code as a plain one (the leaf's node is selected,
 * the sign applied afterwards): every in-line copy of an operand is one plane / sphere / squaroid routine, not two. */
template< int L, class SR, class CT > DEV int operand_side( SR sc, int c, V3 pos, CT* cnt )
{
    const auto cn = &sc.nodes[ c ];
    cnt->inc( CNT_SIDE );
    if( node_has_env( cn ) && env_side( cn, pos, cnt ) == 1 ) return 1;
    if constexpr( L > 1 ) { if( cn->flags & ACN_GFLAG_LEAF_PAIR ) return pair_side< L - 1 >( sc, cn, pos, cnt ); }
    const bool neg = cn->type == ACN_NEG;
    const auto g = neg ? &sc.nodes[ cn->child0 ] : cn;
    if( neg )
    {
        cnt->inc( CNT_SIDE );
        if( node_has_env( g ) && env_side( g, pos, cnt ) == 1 ) return -1;
    }
    const int r = simple_leaf_side( g, pos, cnt );
    return neg ? -r : r;
}

template< class NP, class CT > DEV double simple_leaf_hit( NP g, V3 rp, V3 rd, bool want_nor, V3* nor, CT* cnt )
{
    int type = g->type;
    double a;
    if( type == ACN_PLANE )       a = plane_ray_hit( ld3( g->pos ), ld3( g->rax + 6 ), rp, rd, want_nor, nor, cnt );
    else if( type == ACN_SPHERE ) a = sphere_ray_hit( ld3( g->pos ), g->prm[ 0 ], rp, rd, want_nor, nor, cnt );
    else                          a = squaroid_ray_hit( g, rp, rd, want_nor, nor, cnt );
    if( want_nor && a < F3_INF && g->surface_roughness > 0 ) *nor = roughness_normal( g, *nor, ray_pos( rp, rd, a ), cnt );
    return a;
}

template< int L, bool SPLIT = false, class SR, class O, class CT > DEV double operand_hit( SR sc, int c, O rp, V3 rd, bool want_nor, V3* nor, CT* cnt )
{
    const auto cn = &sc.nodes[ c ];
    cnt->inc( CNT_OBJ_HIT );
    if( node_has_env( cn ) && !env_ray_hits( cn, org_get( rp ), rd, cnt ) ) return F3_INF;
    if constexpr( L > 1 )
    {
        if( cn->flags & ACN_GFLAG_LEAF_PAIR )
        {
            double a = pair_hit< L - 1, SPLIT >( sc, cn, rp, rd, want_nor, nor, cnt );
            if( want_nor && a < F3_INF && cn->surface_roughness > 0 ) *nor = roughness_normal( cn, *nor, ray_pos( org_get( rp ), rd, a ), cnt );
            return a;
        }
    }
    const bool neg = cn->type == ACN_NEG;
    const auto g = neg ? &sc.nodes[ cn->child0 ] : cn;
    if( neg )
    {
        cnt->inc( CNT_OBJ_HIT );
        if( node_has_env( g ) && !env_ray_hits( g, org_get( rp ), rd, cnt ) ) return F3_INF;
    }
    const double a = simple_leaf_hit( g, org_get( rp ), rd, want_nor, nor, cnt );
    if( neg && a < F3_INF && want_nor )
    {
        *nor = v_neg( *nor );                                                                  /* objects.c:1329-1339 */
        if( cn->surface_roughness > 0 ) *nor = roughness_normal( cn, *nor, ray_pos( org_get( rp ), rd, a ), cnt );
    }
    return a;
}

template< int L, class SR, class NP, class CT > DEV int pair_side( SR sc, NP n, V3 pos, CT* cnt )
{
    int want = ( n->type == ACN_PAIR_INSIDE ) ? -1 : 1;
    if( operand_side< L >( sc, n->child0, pos, cnt ) != want ) return -want;
    return operand_side< L >( sc, n->child1, pos, cnt ) == want ? want : -want;
}

/* the pair's hit without its own envelope test and roughness (the caller does both, as for any node): objects.c:1052-1094 /
 * 1209-1251.  The operands' code is expanded in line (calls spill: level-1 operands as real calls cost 69.4 vs 57.4 ms on c2),
 * and how often decides the size of the machine kernels, which do not fit the instruction cache:
 * SPLIT: the pair node is the same in every lane (a root element tested by k_shade, every pair the lock-step machines evaluate):
 * the operand at hand is chosen by a SCALAR index -- its node stays wave-uniform, i.e. scalar loads from the scalar cache instead of
 * a dozen per-lane vector loads per step -- and each of the three places where the reference evaluates "one operand, then the
 * other" (both hits, the two candidate tests, a round of the alternating walk) is a two-trip scalar loop over ONE copy of the
 * operand code, entered by the lanes whose turn it is: two copies of operand_hit and two of operand_side per pair where
 * round 3 had four of each, a quarter of the code two levels deep.  A lane's own sequence of evaluations, and with it every
 * bit of its result, is the reference's. */
template< int L, bool SPLIT, class SR, class NP, class O, class CT > DEV double pair_hit( SR sc, NP n, O rp, V3 rd, bool want_nor, V3* nor, CT* cnt )
{
    const int want = ( n->type == ACN_PAIR_INSIDE ) ? -1 : 1;
    const int c0 = n->child0, c1 = n->child1;
    if constexpr( SPLIT )
    {
        V3 n1 = mk( 0, 0, 0 ), n2 = mk( 0, 0, 0 );
        double a1 = F3_INF, a2 = F3_INF;
        #pragma unroll 1
        for( int k = 0; k < 2; k++ )
        {
            V3 nn = mk( 0, 0, 0 );
            const double aa = operand_hit< L, SPLIT >( sc, k ? c1 : c0, rp, rd, want_nor, &nn, cnt );
            if( k ) { a2 = aa; n2 = nn; } else { a1 = aa; n1 = nn; }
        }
        /* the two candidates: a1 if it is the nearer one and lies on the wanted side of operand 1, else a2 against operand 0 */
        bool open = true;          /* the lane has no result yet */
        double res = F3_INF;
        #pragma unroll 1
        for( int k = 0; k < 2; k++ )
        {
            if( k && open && a2 >= F3_INF ) open = false;   /* res = f3_inf */
            const bool m = k ? open : a1 < a2;
            if( m )
            {
                cnt->cost( ACN_F_PAIR_STEP );
                const double ac = k ? a2 : a1;
                if( operand_side< L >( sc, k ? c0 : c1, ray_pos( org_get( rp ), rd, ac ), cnt ) == want ) { open = false; res = ac; if( want_nor ) *nor = k ? n2 : n1; }
            }
            else if( !k ) cnt->cost( ACN_F_PAIR_STEP );
        }
        if( !open ) return res;
        /* the alternating walk: operand 0 from the far candidate on, then operand 1, ... until a hit lies on the wanted side of
         * the other operand.  A round of the wave serves the lanes whose turn is operand 0, then those whose turn is operand 1 */
        double offs = a2;
        bool swapped = false;
        for( ;; )
        {
            const V3 walk_p = ray_pos( org_get( rp ), rd, offs );
            double a = F3_INF;
            int sd = 0;
            #pragma unroll 1
            for( int k = 0; k < 2; k++ )
            {
                if( swapped == ( k != 0 ) )
                {
                    a = operand_hit< L, SPLIT >( sc, k ? c1 : c0, walk_p, rd, want_nor, &n1, cnt );
                    if( a < F3_INF ) sd = operand_side< L >( sc, k ? c0 : c1, ray_pos( walk_p, rd, a ), cnt );
                }
            }
            cnt->cost( ACN_F_PAIR_STEP );
            if( a >= F3_INF ) return F3_INF;
            if( sd == want ) { if( want_nor ) *nor = n1; return offs + a; }
            offs += a + 2 * F3_EPS;
            if( !( offs < F3_INF ) ) return F3_INF;
            swapped = !swapped;
        }
    }
    else
    {
        V3 n1 = mk( 0, 0, 0 ), n2 = mk( 0, 0, 0 );
        double a1 = operand_hit< L, SPLIT >( sc, c0, rp, rd, want_nor, &n1, cnt );
        double a2 = operand_hit< L, SPLIT >( sc, c1, rp, rd, want_nor, &n2, cnt );
        cnt->cost( ACN_F_PAIR_STEP );
        if( a1 < a2 && operand_side< L >( sc, c1, ray_pos( org_get( rp ), rd, a1 ), cnt ) == want ) { *nor = n1; return a1; }
        if( a2 >= F3_INF ) return F3_INF;
        cnt->cost( ACN_F_PAIR_STEP );
        if( operand_side< L >( sc, c0, ray_pos( org_get( rp ), rd, a2 ), cnt ) == want ) { *nor = n2; return a2; }
        double offs = a2;
        bool swapped = false;
        for( ;; )
        {
            V3 walk_p = ray_pos( org_get( rp ), rd, offs );
            double a = operand_hit< L, SPLIT >( sc, swapped ? c1 : c0, walk_p, rd, want_nor, &n1, cnt );
            cnt->cost( ACN_F_PAIR_STEP );
            if( a >= F3_INF ) return F3_INF;
            int sd = operand_side< L >( sc, swapped ? c0 : c1, ray_pos( walk_p, rd, a ), cnt );
            if( sd == want ) { *nor = n1; return offs + a; }
            offs += a + 2 * F3_EPS;
            if( !( offs < F3_INF ) ) return F3_INF;
            swapped = !swapped;
        }
    }
}

template< class SR, class NP, class CT > DEV int leaf_pair_side( SR sc, NP n, V3 pos, CT* cnt ) { return pair_side< 1 >( sc, n, pos, cnt ); }
template< class SR, class NP, class CT > DEV double leaf_pair_hit( SR sc, NP n, V3 rp, V3 rd, bool want_nor, V3* nor, CT* cnt ) { return pair_hit< 1 >( sc, n, rp, rd, want_nor, nor, cnt ); }
/* the same for a pair node that is the same in every lane */
template< class SR, class NP, class CT > DEV double leaf_pair_hit_uniform( SR sc, NP n, V3 rp, V3 rd, bool want_nor, V3* nor, CT* cnt ) { return pair_hit< 1, true >( sc, n, rp, rd, want_nor, nor, cnt ); }

#endif /* ACN_DEV_LEAVES_H */
