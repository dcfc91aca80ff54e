/* acn_dev_shading.h -- what a shading point needs of a light and of a surface: the cone a light is seen in, the Oren-Nayar weights
 * and the colour of an object at a point. */
#ifndef ACN_DEV_SHADING_H
#define ACN_DEV_SHADING_H

#include "acn_dev_leaves.h"

#pragma clang fp contract(off)

/* ---- fov of a light: objects.c:254-259 -> :520-527, :619-637, :1035-1045 ---- */
DEV void sphere_fov( V3 center, double radius, V3 pos, V3* dir, double* cos_rs )
{
    V3 diff = v_sub( center, pos );
    *dir = v_of_length( diff, 1.0 );
    double diff_sqr = v_sqr( diff );
    double radius_sqr = f_sqr( radius );
    *cos_rs = ( diff_sqr > radius_sqr ) ? acn_sqrt( 1.0 - ( radius_sqr / diff_sqr ) ) : -1;
}

template< class NP > DEV void obj_fov_dev( NP o, V3 pos, V3* dir, double* cos_rs )
{
    if( o->type == ACN_PLANE )
    {
        *dir = v_neg( ld3( o->rax + 6 ) );
        *cos_rs = v_mlv( v_sub( ld3( o->pos ), pos ), *dir ) > 0 ? 0 : 1;
    }
    else if( o->type == ACN_SPHERE )
    {
        sphere_fov( ld3( o->pos ), o->prm[ 0 ], pos, dir, cos_rs );
    }
    else if( node_has_env( o ) )
    {
        sphere_fov( ld3( o->env_pos ), o->env_radius, pos, dir, cos_rs );
    }
    else
    {
        *dir = v_of_length( v_sub( ld3( o->pos ), pos ), 1.0 );
        *cos_rs = 0;
    }
}

/* oren_nayar_weight (scene.c:394-416: sin( max( theta_i, theta_r ) ) * tan( min( theta_i, theta_r ) )) with sin / cos of theta_i
 * supplied by the caller (one value per shading point, many samples): of the two angles only theta_r changes per sample, so one
 * of the reference's two sincos evaluations is loop invariant.  Bit-identical: the values used are the same function results. */
DEV double oren_nayar_weight_pre( double weight, double theta_i, double sin_i, double cos_i, double on_a, double on_b, V3 out_d, V3 nor, V3 ray_prj )
{
    double theta_r = acn_acos( weight );
    double cos_phi = -v_mlv( v_of_length( v_orthogonal_projection( out_d, nor ), 1.0 ), ray_prj );
    double sr, cr;
    acn_sincos( theta_r, &sr, &cr );
    bool i_is_max = !( theta_i < theta_r );          /* f_max( theta_i, theta_r ) == theta_i (a > b ? a : b picks b on a tie) */
    double s1 = i_is_max ? sin_i : sr;
    double s2 = i_is_max ? sr : sin_i;
    double c2 = i_is_max ? cr : cos_i;
    return weight * ( on_a + ( on_b * f_max( cos_phi, 0 ) * s1 * ( s2 / c2 ) ) );
}

/* The same weight for the DIRECT-LIGHT loop (scene.c:556-576), without transcendentals.  There the weight reaches cl_sum and
 * nothing else -- no intensity, sample count, seed or branch -- so it need not carry the rounding of acos / sin / tan, only
 * their value.  With w = weight = out_d . nor (unit vectors), theta_r = acos( w ):
 *     cos( theta_r ) = w,   sin( theta_r ) = sr = sqrt( 1 - w^2 ) = | out_d - nor * w |   (the length v_of_length divides by),
 *     theta_i < theta_r  <=>  cos_i > w,
 *     cos_phi = m / sr   with   m = -( out_d - nor * w ) . ray_prj,
 * hence  max( cos_phi, 0 ) * sin( max ) * tan( min )  =  theta_i >= theta_r:  ( m+ / sr ) * sin_i * ( sr / w ) = m+ * sin_i / w
 *                                                        theta_i <  theta_r:  ( m+ / sr ) * sr * tan_i       = m+ * tan_i
 * and the weight is  w * on_a + on_b * m+ * ( cos_i <= w ? sin_i : w * tan_i ):  eleven multiply-adds and a select instead of
 * acos + sincos + sqrt + two divisions (16 % of k_shade's time, profiles/r03/NOTES.md section 2).  Agreement with
 * the exact form (oren_nayar_weight_pre), measured (tests/test_stages_cpu.py): |closed - exact| <= K 2^-53 on_b / min( sr, cos_i, 1 )
 * with K < 9 -- 6e-14 relative in general, but 7e-10 where out_d lies within 1e-3 rad of the normal (sr < 1e-3, w ~ 1: acos( w )
 * loses the digits of sr) and 3e-13 where theta_i is within 1e-3 of pi / 2; and 5e-9 relative where w < 1e-4, the range in which
 * v_of_length returns its argument unscaled (vectors.h:151), which is the exact form's deviation, not this one's.  The path loop
 * keeps the exact form because its weight becomes the child's intensity (scene.c:596-617).  tan_i is used only where cos_i > w > 0. */
DEV double oren_nayar_weight_direct( double w, double sin_i, double cos_i, double tan_i, double on_a, double on_b, V3 out_d, V3 nor, V3 ray_prj )
{
    double m = -v_mlv( v_orthogonal_projection( out_d, nor ), ray_prj );
    m = f_max( m, 0 );
    return w * on_a + on_b * m * ( cos_i <= w ? sin_i : w * tan_i );
}

/* obj_color (objects.c:411-422): texture field if present (textures.c:99-102, 142-148), else prp.color.
 * obj_projection: plane objects.c:514-518, sphere :602-617, distance :893-896. */
DEV V3 obj_color_dev( const DevScene& sc, int node, V3 pos )
{
    MatP m = &sc.mats[ node ];
    int tex = m->texture;
    if( tex < 0 ) return ld3( m->color );
    TexP t = &sc.textures[ tex ];
    if( t->kind == ACN_TXM_PLAIN ) return ld3( t->color1 );
    NodeP o = &sc.nodes[ node ];
    double px = 0, py = 0;
    if( o->type == ACN_PLANE )
    {
        V3 p = v_sub( pos, ld3( o->pos ) );
        px = v_mlv( p, ld3( o->rax ) );
        py = v_mlv( p, ld3( o->rax + 3 ) );
    }
    else if( o->type == ACN_SPHERE )
    {
        V3 r = v_of_length( v_sub( pos, ld3( o->pos ) ), 1.0 );
        double x = v_mlv( r, ld3( o->rax ) );
        double y = v_mlv( r, v_mlx( ld3( o->rax + 6 ), ld3( o->rax ) ) );
        double z = v_mlv( r, ld3( o->rax + 6 ) );
        px = acn_atan2( x, y );
        z = z >  1.0 ?  1.0 : z;
        z = z < -1.0 ? -1.0 : z;
        py = acn_asin( z );
    }
    long long x = acn_llrint( px * t->scale );
    long long y = acn_llrint( py * t->scale );
    return ( ( x ^ y ) & 1 ) ? ld3( t->color1 ) : ld3( t->color2 );
}

#endif /* ACN_DEV_SHADING_H */
