/* acn_dev_image.h -- raster space: the saturation of a colour, the camera ray of a sample position, the camera basis and the
 * projection of a point.  What the kernels that trace nothing (lens reductions, denoise, reprojection) use beside base and scene. */
#ifndef ACN_DEV_IMAGE_H
#define ACN_DEV_IMAGE_H

#include "acn_dev_base.h"
#include "acn_dev_scene.h"

#pragma clang fp contract(off)

/* vectors.h:372-384 */
DEV V3 cl_sat( V3 o, double gamma )
{
    double x = acn_pow( o.x, gamma );
    double y = acn_pow( o.y, gamma );
    double z = acn_pow( o.z, gamma );
    x = x > 0.0 ? x < 1.0 ? x : 1.0 : 0.0;
    y = y > 0.0 ? y < 1.0 ? y : 1.0 : 0.0;
    z = z > 0.0 ? z < 1.0 ? z : 1.0 : 0.0;
    return mk( x, y, z );
}

/* camera ray for a sample position: scene.c:980-990 */
template< class SC > DEV void camera_ray( const SC& sc, double monitor_x, double monitor_y, V3* rp, V3* rd )
{
    uint64_t width = sc.prm.image_width, height = sc.prm.image_height;
    double z = sc.unit_f * ( ( height >> 1 ) - monitor_y );
    double x = sc.unit_f * ( monitor_x - ( width >> 1 ) );
    V3 d = v_of_length( mk( x, sc.prm.camera_focal_length, z ), 1.0 );
    *rp = ld3( sc.prm.camera_position );
    *rd = m_mlv( sc.camera_rotation, d );
}

/* the camera basis of a set of render parameters with the oracle's expressions (scene.c:963-973): what k_camera_setup stores as
 * DevScene.camera_rotation, and what k_reproject forms per lane for the camera of the previous frame */
DEV M3 camera_rotation_of( const acn_params& prm )
{
    V3 ry = v_of_length( ld3( prm.camera_view_direction ), 1 );
    V3 rz = v_of_length( ld3( prm.camera_top_direction ), 1 );
    rz = v_von( ry, rz );
    V3 rx = v_mlx( ry, rz );
    M3 r; r.x = rx; r.y = ry; r.z = rz;
    return m_transposed( r );
}

/* a pinhole camera as acn_project_points reads it (include/actinon_hip.h): position, right, view and top direction, focal length,
 * half the raster's height and width */
struct ProjCam { V3 pos, R, V, T; double focal, hh, hw; };

DEV ProjCam proj_cam( const M3& rot, const acn_params& prm )
{
    ProjCam c;
    c.pos = ld3( prm.camera_position );
    c.R = m_mlv( rot, mk( 1, 0, 0 ) );
    c.V = m_mlv( rot, mk( 0, 1, 0 ) );
    c.T = m_mlv( rot, mk( 0, 0, 1 ) );
    c.focal = prm.camera_focal_length;
    c.hh = ( double )( prm.image_height >> 1 );
    c.hw = ( double )( prm.image_width >> 1 );
    return c;
}

/* the projection of P: *ly the depth along the view direction, ( *qx, *qy ) the sample position; PROJECTED is the return value */
DEV bool project_point( const ProjCam& c, V3 P, double* qx, double* qy, double* ly )
{
    const V3 v = v_sub( P, c.pos );
    *ly = v_mlv( v, c.V );
    const double s = c.focal / *ly;
    *qx = ( v_mlv( v, c.R ) * s ) * c.hh + c.hw;
    *qy = c.hh - ( v_mlv( v, c.T ) * s ) * c.hh;
    return *ly > 0.0 && __builtin_isfinite( *qx ) && __builtin_isfinite( *qy );
}

#endif /* ACN_DEV_IMAGE_H */
