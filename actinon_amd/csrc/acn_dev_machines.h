/* acn_dev_machines.h -- the two CSG machines, per lane (obj_side_dev, obj_ray_hit_dev) and, through acn_unimachine.h, in lock step. */
#ifndef ACN_DEV_MACHINES_H
#define ACN_DEV_MACHINES_H

#include "acn_dev_leaves.h"

#pragma clang fp contract(off)

/* ------------------------------------------------------------------------------------------------------------------ */
/* CSG machines.  obj_side and obj_ray_hit recurse through pair / neg / scale nodes in the reference; here they are
 * per-lane state machines.  The innermost composite's frame lives in registers; enclosing frames sit on a per-lane
 * stack.  Stack traffic is scratch traffic, and at full occupancy scratch does not fit L2 -- round-1 profiles showed
 * the machine kernels moving ~390 GB per 1080p frame through HBM at 3.7-4.7 TB/s, i.e. bound by their own stacks.
 * Frames are therefore as small as the algorithm allows:
 *   side frame  4 B   node << 2 | pc.  The position is the same for every frame unless a scale wrapper intervenes;
 *                     a scale wrapper parks the outer position on a small auxiliary stack.
 *   hit frame  12 B   node / pc / swapped / inherit packed into one word + ONE double: a1 while the second child is
 *                     evaluated (pc 2), the walk offset afterwards (pc 3), d_factor for a scale wrapper
 *             +24 B   n1, only when normals are wanted (transition hits; never for occlusion tests).
 *   The origin a frame received is not stored: a child evaluated at its parent's own origin inherits it (the common
 *   case); only children entered from the alternating walk or below a scale wrapper park the parent's origin (and the
 *   wrapper its direction) on the auxiliary stack. */
#define ACN_PACK_SIDE( node, pc ) ( ( ( uint32_t )( node ) << 2 ) | ( uint32_t )( pc ) )

template< class SR, class CT >
DEV int obj_side_dev( SR sc, int root, V3 pos, CT* cnt )
{
    uint32_t st[ ACN_CSG_MAX_DEPTH ];
    V3 aux[ ACN_CSG_MAX_DEPTH ];
    const bool lds = sc.lds_stack != ACN_NO_LDS_STACK;
    LdsU32P ls = ( LdsU32P )( ( char ACN_LDS* )acn_lds_raw + sc.lds_stack ) + ACN_LDS_DEPTH * ACN_LDS_LANES * 9 + threadIdx.x;
    uint32_t cur = 0;
    int depth = 0, na = 0;
    int node = root;
    int r = 1;
    ACN_LAP( PH_M_FRAME );
    for( ;; )
    {
        /* EVAL( node, pos ) */
        auto n = &sc.nodes[ node ];
        cnt->inc( CNT_SIDE );
        bool have = true;
        int type = n->type;
        if( node_has_env( n ) && env_side( n, pos, cnt ) == 1 )
        {
            r = 1;
        }
        else if( type <= ACN_DISTANCE )
        {
            switch( type )
            {
                case ACN_PLANE:    cnt->cost( ACN_F_SIDE_PLANE ); r = v_sub_mlv( pos, ld3( n->pos ), ld3( n->rax + 6 ) ) > 0 ? 1 : -1; break;   /* gmath.h:52-55 */
                case ACN_SPHERE:   r = sphere_observer_side( ld3( n->pos ), n->prm[ 0 ], pos, cnt ); break;
                case ACN_SQUAROID: r = squaroid_side( n, pos, cnt ); break;
                default:           r = distance_side( n, pos, cnt ); cnt->inc( CNT_SDF_EVAL ); break;
            }
        }
        else if( n->flags & ACN_GFLAG_LEAF_PAIR )
        {
            r = leaf_pair_side( sc, n, pos, cnt );
        }
        else if( n->flags & ACN_GFLAG_PAIR2 )
        {
            r = pair_side< 2 >( sc, n, pos, cnt );
        }
        else if( depth >= ACN_CSG_MAX_DEPTH )
        {
            atomicOr( sc.flags, ACN_FLAG_STACK_OVERFLOW );
            r = 1;
        }
        else
        {
            if( depth > 0 )
            {
                if( lds && depth <= ACN_LDS_DEPTH ) ls[ ( depth - 1 ) * ACN_LDS_LANES ] = cur; else st[ depth - 1 ] = cur;
            }
            depth++;
            cur = ACN_PACK_SIDE( node, 1 );
            if( type == ACN_SCALE )   /* objects.c:1439-1443 */
            {
                cnt->cost( ACN_F_SIDE_SCALE );
                aux[ na++ ] = pos;    /* na <= depth <= ACN_CSG_MAX_DEPTH */
                M3 rax = node_rax( n );
                V3 p = m_mlv( rax, v_sub( pos, ld3( n->pos ) ) );
                pos = v_mld( p, mk( n->prm[ 0 ], n->prm[ 1 ], n->prm[ 2 ] ) );
            }
            node = n->child0;
            have = false;
        }
        /* RETURN( r ) into the enclosing composites */
        while( have )
        {
            if( depth == 0 ) { ACN_LAP( PH_M_SIDE ); return r; }
            int cnode = ( int )( cur >> 2 );
            auto fn = &sc.nodes[ cnode ];
            int ftype = fn->type;
            bool done = true;
            if( ftype == ACN_NEG ) r = -r;                                   /* objects.c:1341-1344 */
            else if( ftype == ACN_SCALE ) pos = aux[ --na ];
            else
            {
                int want = ( ftype == ACN_PAIR_INSIDE ) ? -1 : 1;           /* objects.c:1096-1099, 1253-1256 */
                if( ( cur & 3u ) == 1u )
                {
                    if( r != want ) r = -want;
                    else { cur = ACN_PACK_SIDE( cnode, 2 ); node = fn->child1; done = false; have = false; }
                }
                else
                {
                    r = ( r == want ) ? want : -want;
                }
            }
            if( done )
            {
                depth--;
                if( depth > 0 ) cur = ( lds && depth <= ACN_LDS_DEPTH ) ? ls[ ( depth - 1 ) * ACN_LDS_LANES ] : st[ depth - 1 ];
            }
        }
    }
}

/* ------------------------------------------------------------------------------------------------------------------ */
/* hit machine: obj_ray_hit (objects.c:261-284) with pair / neg / scale recursion unrolled into frames */
#define ACN_HW_PC( w )       ( ( w ) & 3u )
#define ACN_HW_SWAPPED( w )  ( ( ( w ) >> 2 ) & 1u )
#define ACN_HW_INHERIT( w )  ( ( ( w ) >> 3 ) & 1u )
#define ACN_HW_NODE( w )     ( ( int )( ( w ) >> 4 ) )
#define ACN_HW_PACK( node, pc, swapped, inherit ) ( ( ( uint32_t )( node ) << 4 ) | ( ( uint32_t )( inherit ) << 3 ) | ( ( uint32_t )( swapped ) << 2 ) | ( uint32_t )( pc ) )


template< class SR, class CT >
DEV double obj_ray_hit_dev( SR sc, int root, V3 rp, V3 rd, bool want_nor, V3* out_nor, CT* cnt )
{
    uint32_t st_w[ ACN_CSG_MAX_DEPTH ];
    double   st_a[ ACN_CSG_MAX_DEPTH ];
    V3       st_n[ ACN_CSG_MAX_DEPTH ];     /* touched only when want_nor */
    V3       aux[ 2 * ACN_CSG_MAX_DEPTH ];  /* parked origins / directions */
    const bool lds = sc.lds_stack != ACN_NO_LDS_STACK;
    LdsF64P la = ( LdsF64P )( ( char ACN_LDS* )acn_lds_raw + sc.lds_stack ) + threadIdx.x;
    LdsF64P ln = la + ACN_LDS_DEPTH * ACN_LDS_LANES;   /* x, y, z planes of the parked normals */
    LdsU32P lw = ( LdsU32P )( ( char ACN_LDS* )acn_lds_raw + sc.lds_stack ) + ACN_LDS_DEPTH * ACN_LDS_LANES * 8 + threadIdx.x;
    uint32_t cur_w = 0;
    double cur_a = 0;                       /* pair: a1 (pc 2), walk offset (pc 3) | scale: d_factor */
    V3 cur_n1 = mk( 0, 0, 0 );
    V3 cur_rp = rp;                         /* origin of the ray the current frame received */
    bool rp_derived = false;                /* rp differs from cur_rp (set by the walk and by scale wrappers) */
    int depth = 0, na = 0;
    int node = root;
    double ret_a = F3_INF;
    V3 ret_n = mk( 0, 0, 0 );
    for( ;; )
    {
        /* ---- EVAL( node, rp, rd ) ---- */
        ACN_LAP( PH_M_FRAME );
        auto n = &sc.nodes[ node ];
        cnt->inc( CNT_OBJ_HIT );
        bool have = true;
        int type = n->type;
        if( node_has_env( n ) && !env_ray_hits( n, rp, rd, cnt ) )
        {
            ret_a = F3_INF;
        }
        else if( type <= ACN_DISTANCE )
        {
            switch( type )
            {
                case ACN_PLANE:    ret_a = plane_ray_hit( ld3( n->pos ), ld3( n->rax + 6 ), rp, rd, want_nor, &ret_n, cnt ); break;
                case ACN_SPHERE:   ret_a = sphere_ray_hit( ld3( n->pos ), n->prm[ 0 ], rp, rd, want_nor, &ret_n, cnt ); break;
                case ACN_SQUAROID: ret_a = squaroid_ray_hit( n, rp, rd, want_nor, &ret_n, cnt ); break;
                default:           { V3 dn = mk( 0, 0, 0 ); ret_a = distance_ray_hit( n, rp, rd, want_nor, &dn, cnt ); if( want_nor && ret_a < F3_INF ) ret_n = dn; } break;   /* (a real call: only dn's address escapes, ret_n stays in registers) */
            }
            if( want_nor && ret_a < F3_INF && n->surface_roughness > 0 ) ret_n = roughness_normal( n, ret_n, ray_pos( rp, rd, ret_a ), cnt );
            ACN_LAP( PH_M_LEAF );
        }
        else if( n->flags & ( ACN_GFLAG_LEAF_PAIR | ACN_GFLAG_PAIR2 ) )
        {
            ret_a = ( n->flags & ACN_GFLAG_PAIR2 ) ? pair_hit< 2 >( sc, n, rp, rd, want_nor, &ret_n, cnt )
                                                   : pair_hit< 1 >( sc, n, rp, rd, want_nor, &ret_n, cnt );
            if( want_nor && ret_a < F3_INF && n->surface_roughness > 0 ) ret_n = roughness_normal( n, ret_n, ray_pos( rp, rd, ret_a ), cnt );
            ACN_LAP( PH_M_PAIR );
        }
        else if( depth >= ACN_CSG_MAX_DEPTH )
        {
            atomicOr( sc.flags, ACN_FLAG_STACK_OVERFLOW );
            ret_a = F3_INF;
        }
        else
        {
            if( depth > 0 )
            {
                if( lds && depth <= ACN_LDS_DEPTH )
                {
                    const int o = ( depth - 1 ) * ACN_LDS_LANES;
                    lw[ o ] = cur_w; la[ o ] = cur_a;
                    if( want_nor ) { ln[ o ] = cur_n1.x; ln[ o + ACN_LDS_DEPTH * ACN_LDS_LANES ] = cur_n1.y; ln[ o + 2 * ACN_LDS_DEPTH * ACN_LDS_LANES ] = cur_n1.z; }
                }
                else
                {
                    st_w[ depth - 1 ] = cur_w; st_a[ depth - 1 ] = cur_a;
                    if( want_nor ) st_n[ depth - 1 ] = cur_n1;
                }
            }
            depth++;
            if( rp_derived ) aux[ na++ ] = cur_rp;      /* na <= 2 * depth */
            cur_w = ACN_HW_PACK( node, 1, 0, rp_derived ? 0 : 1 );
            cur_rp = rp;
            rp_derived = false;
            if( type == ACN_SCALE )   /* objects.c:1418-1428 */
            {
                cnt->cost( ACN_F_SCALE_WRAP );
                M3 rax = node_rax( n );
                V3 inv_scale = mk( n->prm[ 0 ], n->prm[ 1 ], n->prm[ 2 ] );
                V3 p2 = v_mld( m_mlv( rax, v_sub( rp, ld3( n->pos ) ) ), inv_scale );
                V3 d2 = v_mld( m_mlv( rax, rd ), inv_scale );
                double d_length = acn_sqrt( v_sqr( d2 ) );
                double d_factor = ( d_length > 0 ) ? ( 1.0 / d_length ) : 0;
                d2 = v_mlf( d2, d_factor );
                aux[ na++ ] = rd; cur_a = d_factor;
                rp = p2; rd = d2;
                rp_derived = true;
            }
            node = n->child0;
            have = false;
        }

        /* ---- RETURN( ret_a, ret_n ) into the enclosing composites ---- */
        while( have )
        {
            if( depth == 0 )
            {
                /* like the reference, the caller's normal is only written on a hit (obj_ray_exit relies on it) */
                if( want_nor && ret_a < F3_INF ) *out_nor = ret_n;
                ACN_LAP( PH_M_FRAME );
                return ret_a;
            }
            int cnode = ACN_HW_NODE( cur_w );
            auto fn = &sc.nodes[ cnode ];
            int ftype = fn->type;
            bool done = true;
            if( ftype == ACN_NEG )   /* objects.c:1329-1339 */
            {
                if( ret_a < F3_INF ) ret_n = v_neg( ret_n );
            }
            else if( ftype == ACN_SCALE )   /* objects.c:1430-1437 */
            {
                double a1 = ret_a + F3_EPS;
                rd = aux[ --na ];
                if( a1 < F3_INF )
                {
                    if( want_nor )
                    {
                        V3 n1 = v_mld( ret_n, mk( fn->prm[ 0 ], fn->prm[ 1 ], fn->prm[ 2 ] ) );
                        ret_n = v_of_length( m_tmlv( node_rax( fn ), n1 ), 1.0 );
                    }
                    ret_a = a1 * cur_a - F3_EPS;
                }
                else
                {
                    ret_a = F3_INF;
                }
            }
            else   /* pair: objects.c:1052-1094 / 1209-1251 */
            {
                int want = ( ftype == ACN_PAIR_INSIDE ) ? -1 : 1;
                uint32_t pc = ACN_HW_PC( cur_w );
                if( pc == 1 )
                {
                    cur_a = ret_a; cur_n1 = ret_n;
                    cur_w = ACN_HW_PACK( cnode, 2, 0, ACN_HW_INHERIT( cur_w ) );
                    node = fn->child1; rp = cur_rp; rp_derived = false;
                    done = false; have = false;
                }
                else if( pc == 2 )
                {
                    /* a step per candidate looked at, as objects.c:1057-1092 takes them: the first always, the second only when the
                     * first is not taken and a2 is finite (booked inside that test's condition below) */
                    cnt->cost( ACN_F_PAIR_STEP );
                    double a1 = cur_a, a2 = ret_a;
                    if( a1 < a2 && obj_side_dev( sc, fn->child1, ray_pos( cur_rp, rd, a1 ), cnt ) == want )
                    {
                        ret_a = a1; ret_n = cur_n1;
                    }
                    else if( a2 >= F3_INF )
                    {
                        ret_a = F3_INF;
                    }
                    else if( ( cnt->cost( ACN_F_PAIR_STEP ), obj_side_dev( sc, fn->child0, ray_pos( cur_rp, rd, a2 ), cnt ) ) == want )
                    {
                        /* ret_a = a2, ret_n = n2 already */
                    }
                    else
                    {
                        cur_a = a2;   /* the walk offset */
                        cur_w = ACN_HW_PACK( cnode, 3, 0, ACN_HW_INHERIT( cur_w ) );
                        node = fn->child0; rp = ray_pos( cur_rp, rd, cur_a ); rp_derived = true;
                        done = false; have = false;
                    }
                }
                else
                {
                    cnt->cost( ACN_F_PAIR_STEP );
                    double a = ret_a;
                    if( a >= F3_INF )
                    {
                        ret_a = F3_INF;
                    }
                    else
                    {
                        V3 walk_p = ray_pos( cur_rp, rd, cur_a );
                        uint32_t swapped = ACN_HW_SWAPPED( cur_w );
                        int obj2 = swapped ? fn->child0 : fn->child1;
                        if( obj_side_dev( sc, obj2, ray_pos( walk_p, rd, a ), cnt ) == want )
                        {
                            ret_a = cur_a + a;   /* ret_n = n1 of the last child call */
                        }
                        else
                        {
                            cur_a += a + 2 * F3_EPS;
                            if( !( cur_a < F3_INF ) )
                            {
                                ret_a = F3_INF;
                            }
                            else
                            {
                                swapped ^= 1u;
                                cur_w = ACN_HW_PACK( cnode, 3, swapped, ACN_HW_INHERIT( cur_w ) );
                                node = swapped ? fn->child1 : fn->child0;
                                rp = ray_pos( cur_rp, rd, cur_a ); rp_derived = true;
                                done = false; have = false;
                            }
                        }
                    }
                }
            }
            if( done )
            {
                /* POST of the composite itself (objects.c:266-282), then hand its result to its parent */
                rp = cur_rp;
                if( want_nor && ret_a < F3_INF && fn->surface_roughness > 0 ) ret_n = roughness_normal( fn, ret_n, ray_pos( rp, rd, ret_a ), cnt );
                if( !ACN_HW_INHERIT( cur_w ) ) cur_rp = aux[ --na ];
                rp_derived = false;
                depth--;
                if( depth > 0 )
                {
                    if( lds && depth <= ACN_LDS_DEPTH )
                    {
                        const int o = ( depth - 1 ) * ACN_LDS_LANES;
                        cur_w = lw[ o ]; cur_a = la[ o ];
                        if( want_nor ) cur_n1 = mk( ln[ o ], ln[ o + ACN_LDS_DEPTH * ACN_LDS_LANES ], ln[ o + 2 * ACN_LDS_DEPTH * ACN_LDS_LANES ] );
                    }
                    else
                    {
                        cur_w = st_w[ depth - 1 ]; cur_a = st_a[ depth - 1 ];
                        if( want_nor ) cur_n1 = st_n[ depth - 1 ];
                    }
                }
            }
        }
    }
}

#include "acn_unimachine.h"

#endif /* ACN_DEV_MACHINES_H */
