/* acn_dev_traverse.h -- rays against the scene: compounds and simple compounds, the root traversals (occlusion and transition
 * hits) with the resume word, their fast forms for k_shade, the cone cull, and scene_trans_hit_dev. */
#ifndef ACN_DEV_TRAVERSE_H
#define ACN_DEV_TRAVERSE_H

#include "acn_dev_machines.h"
#include "acn_dev_prune.h"

#pragma clang fp contract(off)

/* ------------------------------------------------------------------------------------------------------------------ */
/* compounds: compound.c:215-299 */

/* Generic (per-lane indices) closest hit inside compound `cmp`, recursing into nested compounds with an explicit
 * stack. limit: stop as soon as a hit <= limit is found (any-hit for occlusion: "compound_s_ray_hit( matter ) > a"
 * is false iff some element hits at <= a). */
template< class SR, class CT >
DEVN double compound_ray_hit_dev( SR sc, int cmp, V3 rp, V3 rd, bool want_nor, V3* p_nor, int* hit_obj,
                                  double limit, CT* cnt )
{
    int st_i[ ACN_CMP_MAX_DEPTH ], st_end[ ACN_CMP_MAX_DEPTH ];
    int sp = 0;
    double min_a = F3_INF;
    const int order = limit >= 0 ? ( int )sc.n_elems : 0;   /* any-hit queries walk the cost-ordered copy of elems */
    {
        auto o = &sc.nodes[ cmp ];
        if( node_has_env( o ) && !env_ray_hits( o, rp, rd, cnt ) ) return F3_INF;
        st_i[ 0 ] = o->child0 + order; st_end[ 0 ] = o->child0 + order + o->child1; sp = 1;
    }
    while( sp > 0 )
    {
        if( st_i[ sp - 1 ] >= st_end[ sp - 1 ] ) { sp--; continue; }
        int element = sc.elems[ st_i[ sp - 1 ]++ ];
        auto e = &sc.nodes[ element ];
        if( e->type == ACN_COMPOUND )
        {
            if( node_has_env( e ) && !env_ray_hits( e, rp, rd, cnt ) ) continue;
            if( sp >= ACN_CMP_MAX_DEPTH ) { atomicOr( sc.flags, ACN_FLAG_STACK_OVERFLOW ); continue; }
            st_i[ sp ] = e->child0 + order; st_end[ sp ] = e->child0 + order + e->child1; sp++;
            continue;
        }
        V3 nor;
        double a;
        if( e->type >= ACN_PLANE && e->type <= ACN_SQUAROID )   /* a simple leaf (every element of many_spheres): no need for the machine */
        {
            cnt->inc( CNT_OBJ_HIT );
            a = ( node_has_env( e ) && !env_ray_hits( e, rp, rd, cnt ) ) ? F3_INF : simple_leaf_hit( e, rp, rd, want_nor, &nor, cnt );
        }
        else a = obj_ray_hit_dev( sc, element, rp, rd, want_nor, &nor, cnt );
        if( a < min_a )
        {
            min_a = a;
            if( want_nor ) *p_nor = nor;
            if( hit_obj ) *hit_obj = element;
            if( a <= limit ) return a;
        }
    }
    return min_a;
}

/* true only if every point of the sphere ( env_pos, r ) on the ray lies beyond ray parameter `bound` by a margin that covers
 * the F3_EPS the hit routines subtract and all rounding: the origin is outside the sphere, the sphere lies ahead, and its entry
 * point -s - sqrt( s*s - q ) exceeds bound + margin.  Only called for envelopes the ray hits ( s*s >= q ).  Conservative: a `false`
 * costs a visit, a wrong `true` would cost a hit. */
DEV bool env_behind( V3 env_pos, double r, V3 rp, V3 rd, double bound )
{
    V3 p = v_sub( rp, env_pos );
    double s = v_mlv( p, rd );
    double q = v_sqr( p ) - ( r * r );
    double s2 = s * s;
    double u = ( -s - bound ) - ( 1E-5 + 1E-9 * ( fabs( s ) + fabs( bound ) ) );
    return q > 0 && u > 0 && u * u > ( s2 - q ) + 1E-9 * ( s2 + fabs( q ) );
}

/* Simple compounds: a root element that is a compound whose whole subtree consists of nested compounds and simple
 * leaves (many_spheres: 32 768 spheres under five levels of enveloped compounds).  The upload step lays its subtree
 * out in pre-order as SCEntry records with a skip link per entry (elems[ offset ], elems[ offset + 1 ]: first entry and
 * entry count); compound_s_ray_hit (compound.c:215-243) then is a stackless loop: an enveloped compound that the
 * ray misses is skipped by its link, everything else advances by one.  Same element order as the recursion, so ties
 * between equal distances resolve identically.  No stack, no machine: k_shade runs it in line. */

template< bool NOR, class SC, class CT >
DEV double simple_compound_hit( const SC& sc, int cmp, V3 rp, V3 rd, V3* p_nor, int* hit_obj, double limit, CT* cnt )
{
    int off = sc.elems[ sc.prune_base + ( uint32_t )cmp ];
    int i = sc.elems[ off ];
    const int count = sc.elems[ off + 1 ];
    double min_a = F3_INF;
    if( count <= 0 ) return min_a;
    /* The result is the minimum over the leaves, the FIRST leaf in the reference's order winning a tie -- it does not depend on the
     * order of the walk as long as that rule is kept.  The upload step lays big subtrees out a second time with the children of
     * every compound in reverse order; a ray that runs against the order of the first table (order_dir: the direction along which
     * later children lie, summed over the subtree's compounds) walks the second, meets its near leaves sooner and culls more.  In
     * the reversed table the leaves come in exactly the reverse order, so "first wins" becomes "last visited wins": `<=`. */
    bool rev = false;
    if( !CT::counting )
    {
        const int first_rev = sc.elems[ off + 2 ];
        if( first_rev >= 0 )
        {
            const double* g = sc.sc_spheres + 4 * ( size_t )sc.elems[ off + 3 ];
            rev = v_mlv( rd, mk( g[ 0 ], g[ 1 ], g[ 2 ] ) ) < 0;
            if( rev ) i = first_rev;
        }
    }
    const int end = i + count;
    /* CULL: an entry whose envelope provably contains everything below it (ACN_SC_BOUNDING) and lies wholly behind the best hit so
     * far cannot change the result -- every hit in it is farther, and a farther hit never replaces a nearer one -- so it is treated
     * like a missed envelope.  The reference visits it (compound.c:215-243 has no such test); the counting kernels therefore do,
     * too.  many_spheres, every 16th pixel: see profiles/r04/NOTES.md section 6. */
    constexpr bool CULL = !CT::counting;
    auto leaf = [ & ]( int node, int sph, uint32_t flags ) -> bool   /* true: the occlusion form is done */
    {
        V3 nor = mk( 0, 0, 0 );
        double a;
        if( flags & ACN_SC_SPHERE )   /* the sphere itself from the compact table beside the entries (32 B, L2-resident) instead of its 192-byte node */
        {
            const double* g = sc.sc_spheres + 4 * ( size_t )sph;
            a = sphere_ray_hit( mk( g[ 0 ], g[ 1 ], g[ 2 ] ), g[ 3 ], rp, rd, NOR, &nor, cnt );
            if( NOR && a < F3_INF && ( flags & ACN_SC_ROUGH ) ) nor = roughness_normal( &sc.nodes[ node ], nor, ray_pos( rp, rd, a ), cnt );
        }
        else a = simple_leaf_hit( &sc.nodes[ node ], rp, rd, NOR, &nor, cnt );
        if( rev ? ( a <= min_a && a < F3_INF ) : ( a < min_a ) )
        {
            min_a = a;
            if( NOR ) *p_nor = nor;
            *hit_obj = node;
            if( a <= limit ) return true;
        }
        return false;
    };
    SCEntry e = sc.sc_table[ i ];
    while( i < end )
    {
        bool miss = ( e.flags & ACN_NODE_HAS_ENVELOPE ) && !env_ray_hits_raw( ld3( e.env_pos ), e.env_radius, rp, rd, cnt );
        if( CULL && !miss && ( e.flags & ACN_SC_BOUNDING ) )
        {
            const double bound = NOR ? min_a : limit;   /* the occlusion form leaves at the first hit within `limit`: nothing beyond it matters */
            if( bound < F3_INF ) miss = env_behind( ld3( e.env_pos ), e.env_radius, rp, rd, bound );
        }
        const bool is_leaf = e.type != ACN_COMPOUND;
        const int next = ( !is_leaf && miss ) ? e.skip : i + 1;
        if( is_leaf ) cnt->inc( CNT_OBJ_HIT );
        const bool want = is_leaf && !miss;
        if( want )
        {
            if( leaf( e.node, e.skip, e.flags ) ) return min_a;
        }
        if( next < end ) e = sc.sc_table[ next ];
        i = next;
    }
    return min_a;
}

/* Conservative pruning before a ray is handed to the CSG machine: surely_outside( n ) == true guarantees that the
 * whole ray lies outside n's bounding envelopes, in which case the reference returns f3_inf for n AND obj_side( n )
 * is +1 at every point of the ray:
 *   - n has an envelope and the ray misses it (objects.c:264, :368);
 *   - pair_outside: both children surely outside -> a1 = a2 = f3_inf -> f3_inf (objects.c:1224), side 1+1 == 2;
 *   - pair_inside: one child surely outside -> it returns f3_inf and classifies every point of the ray as outside, so
 *     neither the direct candidates nor the alternating walk can accept a hit (objects.c:1057-1092), side != -2.
 * Complements and scale wrappers are never pruned.  Expanded D levels deep. */
template< int D, class NP >
DEV bool surely_outside_n( NP nodes, int node, V3 rp, V3 rd )
{
    auto n = &nodes[ node ];
    /* levels of this node worth reading (upload step, actinon_hip.hip): 0 nothing to test here or below, 1 only the node's own
     * envelope, ...: the same tests as a blind descent, without the operand reads that lead to no test */
    const uint32_t levels = ( n->flags >> ACN_GFLAG_PRUNE_LEVELS_SHIFT ) & 7u;
    if( levels == 0 ) return false;
    if( node_has_env( n ) && !env_ray_hits( n, rp, rd, ACN_NO_CNT ) ) return true;
    if constexpr( D > 0 )
    {
        if( levels < 2 ) return false;
        int type = n->type;
        if( type == ACN_PAIR_OUTSIDE ) return surely_outside_n< D - 1 >( nodes, n->child0, rp, rd ) && surely_outside_n< D - 1 >( nodes, n->child1, rp, rd );
        if( type == ACN_PAIR_INSIDE )  return surely_outside_n< D - 1 >( nodes, n->child0, rp, rd ) || surely_outside_n< D - 1 >( nodes, n->child1, rp, rd );
    }
    return false;
}
template< int D, class SC >
DEV bool surely_outside( const SC& sc, int node, V3 rp, V3 rd ) { return surely_outside_n< D >( sc.nodes, node, rp, rd ); }

/* Hit test of ROOT element `e` (an index that is the same in every active lane of the wave, so the node is read
 * through the scalar cache into SGPRs and the type dispatch is a scalar branch): obj_ray_hit (objects.c:261-284)
 * for objects -- plane / sphere / squaroid inline, CSG and SDF objects through the hit machine -- and
 * compound_s_ray_hit for nested compounds.
 * pre (per lane): run the pre-tests that can only answer "no hit": the element's envelope, surely_outside and the prune
 * program.  A lane whose ray k_shade has already put through the same tests with the answer "not ruled out" passes false
 * (resumed records, see the fast-path forms below); what is evaluated then is evaluated as ever.  (A generic nested compound
 * keeps its envelope test: it belongs to compound_ray_hit_dev, a real call that k_walk shares.) */
template< bool NOR, class SC, class CT >
DEV double element_hit( const SC& sc, int e, V3 rp, V3 rd, V3* nor, int* hit_obj, double limit, CT* cnt, bool pre = true )
{
    ACN_NODE( n, &sc.nodes[ e ] )
    int type = n->type;
    if( type == ACN_COMPOUND )
    {
        if constexpr( SC::prune )   /* the "extras" kernel variants (DevScenePT) */
        {
            if( n->flags & ACN_GFLAG_SIMPLE_COMPOUND )
            {
                if( pre && node_has_env( n ) && !env_ray_hits( n, rp, rd, cnt ) ) return F3_INF;
                return simple_compound_hit< NOR >( sc, e, rp, rd, nor, hit_obj, limit, cnt );
            }
        }
        ACN_LAP( PH_ROOT_LEAF );
        /* a real call: it gets the addresses of two locals, so that the caller's normal and hit object -- which every other
         * branch of this function writes too -- are not forced into scratch memory by an escaping pointer */
        V3 cn = mk( 0, 0, 0 );
        int co = *hit_obj;
        double ac = compound_ray_hit_dev( sref( sc ), e, rp, rd, NOR, &cn, &co, limit, cnt );   /* (a real call with its own envelope test, whatever pre says) */
        if( ac < F3_INF ) { if constexpr( NOR ) *nor = cn; *hit_obj = co; }
        ACN_LAP( PH_COMPOUND );
        return ac;
    }
    *hit_obj = e;
    bool env = node_has_env( n );
    /* the envelope pre-test.  An element that goes on to a machine has the test redone, and booked, there: here only its miss is an
     * event of the reference (objects.c:264), so the test itself runs without the counters */
    if( pre && env && !( type > ACN_SQUAROID ? env_ray_hits( n, rp, rd, ACN_NO_CNT ) : env_ray_hits( n, rp, rd, cnt ) ) )
    {
        if( type > ACN_SQUAROID ) cnt->cost( ACN_F_ENV_MISS );
        cnt->inc( CNT_OBJ_HIT );
        return F3_INF;
    }
    if( type > ACN_SQUAROID )
    {
#ifdef ACN_PRUNE_CHECK
        if( type != ACN_DISTANCE && surely_outside< ACN_PRUNE_DEPTH >( sc, e, rp, rd ) ) { cnt->inc( CNT_OBJ_HIT ); return F3_INF; }
        {
            bool pr = type != ACN_DISTANCE && prune_run( sc, e, rp, rd, F3_INF );
            V3 nn = mk( 0, 0, 0 );
            double aa = obj_ray_hit_dev( sref( sc ), e, rp, rd, NOR, NOR ? nor : &nn, cnt );
            if( pr && aa < F3_INF ) printf( "PRUNE VIOLATION e=%d a=%.17g rp=%.17g %.17g %.17g rd=%.17g %.17g %.17g\n", e, aa, rp.x, rp.y, rp.z, rd.x, rd.y, rd.z );
            return aa;
        }
#endif
        ACN_LAP( PH_ROOT_LEAF );
        if( pre && type != ACN_DISTANCE && ( surely_outside< ACN_PRUNE_DEPTH >( sc, e, rp, rd ) || prune_run( sc, e, rp, rd, F3_INF ) ) ) { cnt->inc( CNT_OBJ_HIT ); ACN_LAP( PH_PRUNE ); return F3_INF; }
        ACN_LAP( PH_PRUNE );
        return obj_ray_hit_uni< NOR, SC::park >( sref( sc ), e, rp, rd, nor, cnt );   /* the machine redoes the envelope test */
    }
    cnt->inc( CNT_OBJ_HIT );
    double a;
    if( type == ACN_PLANE )       a = plane_ray_hit( ld3( n->pos ), ld3( n->rax + 6 ), rp, rd, NOR, nor, cnt );
    else if( type == ACN_SPHERE ) a = sphere_ray_hit( ld3( n->pos ), n->prm[ 0 ], rp, rd, NOR, nor, cnt );
    else                          a = squaroid_ray_hit( n, rp, rd, NOR, nor, cnt );
    if( NOR && a < F3_INF && n->surface_roughness > 0 ) *nor = roughness_normal( n, *nor, ray_pos( rp, rd, a ), cnt );
    return a;
}

/* obj_ray_hit of a light that is not a plain sphere / plane (k_shade's LEAF_LIGHTS = false variants): a real function
 * call, so that those rarely used kernels do not each carry an in-line copy of the CSG machines */
template< class SC, class CT >
DEVN double light_hit_call( SC sc, int e, V3 rp, V3 rd, CT* cnt )
{
    int ho;
    return element_hit< false >( sc, e, rp, rd, ( V3* )nullptr, &ho, -F3_INF, cnt );
}

/* Resume words.  k_shade's in-line passes over the matter root (root_occluded_fast, root_trans_hit_fast below) tell the hard-ray
 * kernels which root elements are left to do.  A candidate word: bit i, i < ACN_RESUME_POSITIONS: the element at position i of
 * the root's given order ( elems[ child0 + i ] ) is a candidate; bit ACN_RESUME_POSITIONS: so is some element at a position
 * beyond.  In a record (HardShadow.pad, HardPath.resume) the word sits two bits up: bit 0 is the record's own ("the light root
 * counts too"), bit 1 says that the record is resumable at all -- clear: every element is to be done, as for the probes of
 * k_walk, which nothing has looked at. */
#define ACN_RESUME_POSITIONS 29
#define ACN_RESUME_FLAG 2u
DEV uint32_t resume_bit( int i ) { return 1u << ( i < ACN_RESUME_POSITIONS ? i : ACN_RESUME_POSITIONS ); }
DEV uint32_t resume_record( uint32_t candidates ) { return ( candidates << 2 ) | ACN_RESUME_FLAG; }
/* does the record ask for the element at position i ?  (i: wave-uniform) */
DEV bool resume_wants( uint32_t rec, int i ) { return !( rec & ACN_RESUME_FLAG ) || ( ( rec >> 2 ) & resume_bit( i ) ); }
/* ... and does that element still need its pre-tests (element_hit) ?  k_shade has run them at the positions it can name */
DEV bool resume_pre( uint32_t rec, int i ) { return !( rec & ACN_RESUME_FLAG ) || i >= ACN_RESUME_POSITIONS; }

/* compound_s_ray_hit on a root compound, any-hit form for occlusion tests: true iff some element hits at <= limit.
 * RESUME: rec is a record's resume word (lanes with full and with resumed records share the loop and the one in-line copy
 * of the machines in it); an element no lane of the wave asks for is skipped.  elems[ pos_base + k ]: the position, in its
 * compound's given order, of entry k of the cost-ordered copy elems[ n_elems + k ] (written by the upload step). */
template< bool RESUME, class SC, class CT >
DEV bool root_occluded_rec( const SC& sc, int cmp, V3 rp, V3 rd, double limit, uint32_t rec, uint32_t pos_base, CT* cnt )
{
    auto o = &sc.nodes[ cmp ];
    if( ( !RESUME || !( rec & ACN_RESUME_FLAG ) ) && node_has_env( o ) && !env_ray_hits( o, rp, rd, cnt ) ) return false;   /* (k_shade passed it) */
    int first = o->child0 + ( int )sc.n_elems, count = o->child1;   /* the cost-ordered copy: cheap elements first */
    bool occ = false;
    for( int i = 0; i < count; i++ )
    {
        int element = __builtin_amdgcn_readfirstlane( sc.elems[ first + i ] );
        if constexpr( RESUME )
        {
            const int at = __builtin_amdgcn_readfirstlane( sc.elems[ pos_base + ( uint32_t )( o->child0 + i ) ] );
            const bool want = !occ && resume_wants( rec, at );
            if( __ballot( want ) == 0ull ) continue;   /* (some lane is not occluded yet, or the loop had ended) */
            if( want )
            {
                int hit_obj;
                double a = element_hit< false >( sc, element, rp, rd, nullptr, &hit_obj, limit, cnt, resume_pre( rec, at ) );
                if( a <= limit ) occ = true;
            }
        }
        else if( !occ )
        {
            int hit_obj;
            double a = element_hit< false >( sc, element, rp, rd, nullptr, &hit_obj, limit, cnt );
            if( a <= limit ) occ = true;
        }
        if( __ballot( !occ ) == 0ull ) break;
    }
    return occ;
}
template< class SC, class CT >
DEV bool root_occluded( const SC& sc, int cmp, V3 rp, V3 rd, double limit, CT* cnt ) { return root_occluded_rec< false >( sc, cmp, rp, rd, limit, 0u, 0u, cnt ); }

struct Trans { V3 exit_nor; int exit_obj; int enter_obj; };

/* compound_s_ray_trans_hit on a root compound (compound.c:246-299).
 * RESUME: rec is a record's resume word.  The loop keeps the given order and only leaves elements out, all of which are
 * known to miss: the fold below is the full fold without its no-ops. */
template< bool RESUME, class SC, class CT >
DEV double root_trans_hit_rec( const SC& sc, int cmp, V3 rp, V3 rd, Trans* trans, uint32_t rec, CT* cnt )
{
    auto o = &sc.nodes[ cmp ];
    cnt->inc( CNT_TRANS_RAY );
    if( ( !RESUME || !( rec & ACN_RESUME_FLAG ) ) && node_has_env( o ) && !env_ray_hits( o, rp, rd, cnt ) ) return F3_INF;   /* (k_shade passed it) */
    double min_a = F3_INF;
    int first = o->child0, count = o->child1;
    for( int i = 0; i < count; i++ )
    {
        bool want = true, pre = true;
        if constexpr( RESUME )
        {
            want = resume_wants( rec, i ); pre = resume_pre( rec, i );
            if( __ballot( want ) == 0ull ) continue;
        }
        int element = __builtin_amdgcn_readfirstlane( sc.elems[ first + i ] );
        int hit_obj = -1;
        V3 nor = mk( 0, 0, 0 );
        double a = F3_INF;
        if( want ) a = element_hit< true >( sc, element, rp, rd, &nor, &hit_obj, -F3_INF, cnt, pre );
        if( a < F3_INF )
        {
            cnt->cost( ACN_F_TRANS_RESOLVE );
            if( a < min_a - F3_EPS )
            {
                min_a = a;
                if( v_mlv( nor, rd ) > 0 )
                {
                    trans->exit_nor = nor; trans->exit_obj = hit_obj; trans->enter_obj = -1;
                }
                else
                {
                    trans->exit_nor = v_neg( nor ); trans->exit_obj = -1; trans->enter_obj = hit_obj;
                }
            }
            else if( f_abs( a - min_a ) < F3_EPS )
            {
                min_a = a < min_a ? a : min_a;
                if( v_mlv( nor, rd ) > 0 ) trans->exit_obj = hit_obj;
                else                       trans->enter_obj = hit_obj;
            }
        }
    }
    return min_a;
}
template< class SC, class CT >
DEV double root_trans_hit( const SC& sc, int cmp, V3 rp, V3 rd, Trans* trans, CT* cnt ) { return root_trans_hit_rec< false >( sc, cmp, rp, rd, trans, 0u, cnt ); }

/* ---- fast-path forms for k_shade: leaf root elements are tested inline; a ray that gets past the pre-tests of a root
 * element that needs the machine (CSG, SDF, nested compound) is reported as hard and handed to the hard-ray kernels,
 * which RESUME the query where this pass leaves it: the pass returns a candidate word (ACN_RESUME_POSITIONS above) and the
 * hard-ray kernels visit the named elements only, without the pre-tests this pass has run on them.
 *   occlusion    an OR over the elements.  The candidates are the machine elements that were not ruled out.  Every other
 *                element has been evaluated here, or culled for the whole cone, and does not occlude within `limit` -- else
 *                the pass had answered 1 -- so leaving it out of the OR changes nothing.
 *   transition   the fold of compound.c:246-299 ignores an element that misses, but depends on the order of those that
 *                hit within F3_EPS of each other.  The candidates are the machine elements that were not ruled out AND the
 *                in-line elements that hit here; k_hard_path folds them all again, in the given order: the full fold with
 *                the misses left out.  (The fold of this pass is only used when there is no candidate machine element.)
 *   pre-tests    element_hit's envelope test, surely_outside and prune_run( F3_INF ) are what this pass ran on the same
 *                operands with the answer "not ruled out" (prune_run( limit ) == false implies prune_run( F3_INF ) == false:
 *                the limit only cuts the hull); an in-line element that hit has passed its envelope.  Skipping them
 *                skips tests whose outcome is known; what is evaluated is evaluated by the same code as in a full pass.
 *                Positions the word cannot name (the tail bit) keep their pre-tests.
 * A transition hit is only final here when every machine element was missed at its pre-tests (obj_ray_hit then returns
 * f3_inf for it, objects.c:264). ---- */
DEV bool is_fast_type( int type ) { return type >= ACN_PLANE && type <= ACN_SQUAROID; }

template< bool NOR, class NP, class CT >
DEV double leaf_element_hit( NP n, int type, V3 rp, V3 rd, V3* nor, CT* cnt )
{
    cnt->inc( CNT_OBJ_HIT );
    if( node_has_env( n ) && !env_ray_hits( n, rp, rd, cnt ) ) return F3_INF;
    double a;
    if( type == ACN_PLANE )       a = plane_ray_hit( ld3( n->pos ), ld3( n->rax + 6 ), rp, rd, NOR, nor, cnt );
    else if( type == ACN_SPHERE ) a = sphere_ray_hit( ld3( n->pos ), n->prm[ 0 ], rp, rd, NOR, nor, cnt );
    else                          a = squaroid_ray_hit( n, rp, rd, NOR, nor, cnt );
    if( NOR && a < F3_INF && n->surface_roughness > 0 ) *nor = roughness_normal( n, *nor, ray_pos( rp, rd, a ), cnt );
    return a;
}

/* a ROOT element that is a leaf pair: obj_ray_hit (objects.c:261-284) in line, no machine, no deferral */
template< bool NOR, class SC, class NP, class CT >
DEV double leaf_pair_element_hit( const SC& sc, NP n, V3 rp, V3 rd, V3* nor, CT* cnt )
{
    cnt->inc( CNT_OBJ_HIT );
    if( node_has_env( n ) && !env_ray_hits( n, rp, rd, cnt ) ) return F3_INF;
    V3 nn = mk( 0, 0, 0 );
    double a = leaf_pair_hit_uniform( sref( sc ), n, rp, rd, NOR, &nn, cnt );
    if( NOR && a < F3_INF )
    {
        if( n->surface_roughness > 0 ) nn = roughness_normal( n, nn, ray_pos( rp, rd, a ), cnt );
        *nor = nn;
    }
    return a;
}

/* Cone culling of the root elements for the direct-light loop of one shading point (k_shade).  All of a loop's shadow
 * rays start at `pos` and lie inside the cone the light is sampled in: out_d = src_con * sphere_cap( cyl_hgt ) has
 * out_d . axis = 1 - u * cyl_hgt >= cos_theta (scene.c:549-558, vectors.h:197-206).  Bit i of the result: element i of the
 * root compound cannot be hit by ANY ray of that cone -- obj_ray_hit would return f3_inf for every sample -- so the sample
 * loop skips it and every result stays what it was:
 *   - an element with an envelope (objects.c:264: the ray must hit the envelope sphere first), or a sphere leaf: the ball
 *     lies outside the cone when the angle between axis and centre exceeds theta + asin( R / L );
 *   - a plane (gmath.h:38-50): hit iff ( plane.pos - pos ) . nor and nor . rd have the same sign; over the cone nor . rd
 *     stays on one side of zero when the angle between nor and axis differs from 90 degrees by more than theta.
 * Conservative by 1e-9 (directions are unit vectors to ~1e-16); anything uncertain is kept.  Per shading point and
 * light ~40 flop per element instead of ~25 per element AND SAMPLE: on the wine glass a floor point outside the glass's
 * shadow tests nothing per sample (k_shade spent 23 % of its time in the occlusion test, profiles/r03). */
template< class SC >
DEV uint64_t root_cone_cull( const SC& sc, int cmp, V3 pos, V3 axis, double cos_theta )
{
    auto o = &sc.nodes[ cmp ];
    uint64_t skip = 0;
#ifdef ACN_NO_CONE_CULL
    return 0;
#endif
    if( !( cos_theta > 1.0e-6 ) ) return 0;                 /* half space or more (plane lights, points inside a light) */
    const double sin_theta = acn_sqrt( f_max( 0.0, 1.0 - cos_theta * cos_theta ) );
    const int first = o->child0, count = o->child1 < 64 ? o->child1 : 64;
    for( int i = 0; i < count; i++ )
    {
        int element = __builtin_amdgcn_readfirstlane( sc.elems[ first + i ] );
        auto n = &sc.nodes[ element ];
        const int type = n->type;
        bool out = false;
        if( node_has_env( n ) || type == ACN_SPHERE )
        {
            const bool env = node_has_env( n );
            const V3 c = env ? ld3( n->env_pos ) : ld3( n->pos );
            const double R = env ? n->env_radius : n->prm[ 0 ];
            const V3 v = v_sub( c, pos );
            const double L2 = v_sqr( v ), R2 = R * R;
            if( L2 > R2 * ( 1.0 + 1.0e-9 ) + 1.0e-30 )
            {
                const double L = acn_sqrt( L2 );
                const double cos_phi = v_mlv( v, axis ) / L;
                const double sin_alpha = R / L;
                const double cos_alpha = acn_sqrt( f_max( 0.0, 1.0 - sin_alpha * sin_alpha ) );
                const double cos_sum = cos_theta * cos_alpha - sin_theta * sin_alpha;     /* cos( theta + alpha ), theta + alpha < pi */
                out = cos_phi < cos_sum - 1.0e-9;
            }
        }
        else if( type == ACN_PLANE )
        {
            const V3 nor = ld3( n->rax + 6 );
            const double s0 = v_sub_mlv( ld3( n->pos ), pos, nor );
            const double c = v_mlv( nor, axis );                                           /* cos of the angle between nor and axis */
            const double s = acn_sqrt( f_max( 0.0, 1.0 - c * c ) );
            const double d_min = c * cos_theta - s * sin_theta, d_max = c * cos_theta + s * sin_theta;   /* range of nor . rd over the cone */
            out = ( s0 < 0 && d_min > 1.0e-9 ) || ( s0 > 0 && d_max < -1.0e-9 );
        }
        if( out ) skip |= 1ull << i;
    }
    return skip;
}

/* The positions of the root that root_occluded_fast visits, and where it reads the root node's own fields: RootAll is every
 * position in turn and the node itself at every call; k_shade passes the positions some lane of the wave still wants, with
 * the node's fields resolved once per light (RootSet, acn_k_shade.h). */
struct RootAll
{
    template< class NP > DEV bool env( NP o ) const { return node_has_env( o ); }
    template< class NP > DEV int first( NP o ) const { return o->child0; }
    template< class NP > DEV int count( NP o ) const { return o->child1; }
    DEV bool none() const { return false; }
    DEV int begin() const { return 0; }
    DEV int next( int i ) { return i + 1; }
};

/* 0: not occluded, 1: occluded, 2: undecided (hard).  skip: root_cone_cull's bits.  *candidates: where the answer is 2, the
 * machine elements that were not ruled out (a candidate word; it takes the place of a `hard` flag in the loop) */
template< class SC, class CT, class POS = RootAll >
DEV int root_occluded_fast( const SC& sc, int cmp, V3 rp, V3 rd, double limit, uint64_t skip, uint32_t* candidates, CT* cnt, POS at = POS() )
{
    auto o = &sc.nodes[ cmp ];
    *candidates = 0;
    if( !CT::counting && at.none() ) return 0;   /* (the envelope test below decides nothing then; a COUNT variant books it) */
    if( at.env( o ) && !env_ray_hits( o, rp, rd, cnt ) ) return 0;
    int first = at.first( o ), count = at.count( o );
    uint32_t hard = 0;
    for( int i = at.begin(); i < count; i = at.next( i ) )
    {
        if( i < 64 && ( ( skip >> i ) & 1ull ) ) continue;
        int element = __builtin_amdgcn_readfirstlane( sc.elems[ first + i ] );
        ACN_NODE( n, &sc.nodes[ element ] )
        int type = n->type;
        if( is_fast_type( type ) )
        {
            double a = leaf_element_hit< false >( n, type, rp, rd, nullptr, cnt );
            if( a <= limit ) return 1;
        }
        else if( n->flags & ACN_GFLAG_LEAF_PAIR )
        {
            double a = leaf_pair_element_hit< false >( sc, n, rp, rd, nullptr, cnt );
            if( a <= limit ) return 1;
        }
        else if( SC::prune && ( n->flags & ACN_GFLAG_SIMPLE_COMPOUND ) )
        {
            if( node_has_env( n ) && !env_ray_hits( n, rp, rd, cnt ) ) continue;
            int ho;
            double a = simple_compound_hit< false >( sc, element, rp, rd, nullptr, &ho, limit, cnt );
            if( a <= limit ) return 1;
        }
        else if( type == ACN_COMPOUND || type == ACN_DISTANCE ? ( !node_has_env( n ) || env_ray_hits( n, rp, rd, ACN_NO_CNT ) )
                                                              : !( surely_outside< ACN_PRUNE_DEPTH >( sc, element, rp, rd ) || ACN_FAST_PRUNE( sc, element, rp, rd, limit ) ) )
        {
            hard |= resume_bit( i );
        }
    }
    *candidates = hard;
    return hard ? 2 : 0;
}

/* compound_s_ray_trans_hit on a root compound; *hard is set when the query must be finished by the full traversal.
 * *machines: the candidate word of the machine elements that were not ruled out ( != 0 iff *hard ); *inline_hits: that of
 * the in-line elements that hit.  Both together are what k_hard_path folds; an any-hit probe needs the first alone. */
template< class SC, class CT >
DEV double root_trans_hit_fast( const SC& sc, int cmp, V3 rp, V3 rd, Trans* trans, bool* hard, uint32_t* machines, uint32_t* inline_hits, CT* cnt )
{
    auto o = &sc.nodes[ cmp ];
    *hard = false; *machines = 0; *inline_hits = 0;
    if( node_has_env( o ) && !env_ray_hits( o, rp, rd, cnt ) ) { cnt->inc( CNT_TRANS_RAY ); return F3_INF; }
    double min_a = F3_INF;
    int first = o->child0, count = o->child1;
    uint32_t h = 0, hits = 0;
    for( int i = 0; i < count; i++ )
    {
        int element = __builtin_amdgcn_readfirstlane( sc.elems[ first + i ] );
        ACN_NODE( n, &sc.nodes[ element ] )
        int type = n->type;
        if( !is_fast_type( type ) && !( n->flags & ( ACN_GFLAG_LEAF_PAIR | ( SC::prune ? ACN_GFLAG_SIMPLE_COMPOUND : 0u ) ) ) )
        {
            if( type == ACN_COMPOUND || type == ACN_DISTANCE ? ( !node_has_env( n ) || env_ray_hits( n, rp, rd, ACN_NO_CNT ) )
                                                             : !( surely_outside< ACN_PRUNE_DEPTH >( sc, element, rp, rd ) || ACN_FAST_PRUNE( sc, element, rp, rd, F3_INF ) ) ) h |= resume_bit( i );
            continue;
        }
        V3 nor = mk( 0, 0, 0 );
        double a;
        if( is_fast_type( type ) ) a = leaf_element_hit< true >( n, type, rp, rd, &nor, cnt );
        else if( n->flags & ACN_GFLAG_LEAF_PAIR ) a = leaf_pair_element_hit< true >( sc, n, rp, rd, &nor, cnt );
        else
        {
            /* the hit object of a compound is the leaf that was hit (compound.c:225-243) */
            a = F3_INF;
            if constexpr( SC::prune )
            {
                if( !node_has_env( n ) || env_ray_hits( n, rp, rd, cnt ) ) a = simple_compound_hit< true >( sc, element, rp, rd, &nor, &element, -F3_INF, cnt );
            }
        }
        if( a < F3_INF )
        {
            hits |= resume_bit( i );
            cnt->cost( ACN_F_TRANS_RESOLVE );
            if( a < min_a - F3_EPS )
            {
                min_a = a;
                if( v_mlv( nor, rd ) > 0 )
                {
                    trans->exit_nor = nor; trans->exit_obj = element; trans->enter_obj = -1;
                }
                else
                {
                    trans->exit_nor = v_neg( nor ); trans->exit_obj = -1; trans->enter_obj = element;
                }
            }
            else if( f_abs( a - min_a ) < F3_EPS )
            {
                min_a = a < min_a ? a : min_a;
                if( v_mlv( nor, rd ) > 0 ) trans->exit_obj = element;
                else                       trans->enter_obj = element;
            }
        }
    }
    *hard = h != 0; *machines = h; *inline_hits = hits;
    if( !h ) cnt->inc( CNT_TRANS_RAY );
    return min_a;
}

/* ------------------------------------------------------------------------------------------------------------------ */
template< class SC, class CT >
DEV double scene_trans_hit_dev( const SC& sc, V3 rp, V3 rd, Trans* trans, CT* cnt )   /* scene.c:362-382 */
{
    double min_a = F3_INF;
    double a;
    Trans trans_l;
    trans_l.exit_nor = mk( 0, 0, 0 ); trans_l.exit_obj = -1; trans_l.enter_obj = -1;
    ACN_LAP( PH_FETCH );
    /* lights, then matter, through ONE in-line copy of the root traversal (and of the CSG machines in it): the root is a scalar */
    #pragma unroll 1
    for( int k = 0; k < 2; k++ )
    {
        if( ( a = root_trans_hit( sc, k ? sc.matter_root : sc.light_root, rp, rd, &trans_l, cnt ) ) < min_a )
        {
            min_a = a;
            *trans = trans_l;
        }
        if( k == 0 ) ACN_LAP( PH_LIGHT );
    }
    ACN_LAP( PH_ROOT_LEAF );
    return min_a;
}

#endif /* ACN_DEV_TRAVERSE_H */
