/* k_reproject.hip -- acn_project_points*, acn_reproject* and acn_reproject_moving* (include/actinon_hip.h states the projection, the taps,
 * the validity rules, the gather and the motion table; tests/reproject_model.py and tests/motion_model.py restate them in numpy and the
 * two are compared bit for bit).
 *
 *   k_project_points  one point per lane: the inverse of camera_ray with the handle's camera.
 *   k_reproject       one position per lane, as k_stats_merge and k_lens_layers_merge.  The lane reads the six 16-byte pieces of its
 *                  current surface record that the rules read, forms the previous camera's basis from the previous frame's parameters by
 *                  the expressions of k_camera_setup (camera_rotation_of: the same in every lane, a few dozen operations beside 900 bytes
 *                  of traffic), projects, and visits the four taps in order.  A tap is converted to an index and read only after its
 *                  in-image test, made on doubles, and only if its weight is positive: its statistics record as four pieces, the pieces
 *                  of its surface record that the rules read.  The tap loop is unrolled over constant indices, so everything stays in
 *                  registers; no lane reads another lane's registers: a record depends on its current record and four previous positions alone.
 *   k_reproject_moving  the same body (reproject_body< true >) with a motion table: the lane reads piece 6 of the row of its record's
 *                  object -- state and cap, 16 bytes -- and the six pieces of A and t only if the row is MOVED; the table is not staged
 *                  in LDS: rows are gathered by object id, and a table of a few rows sits in the caches.
 * The EMPTY rule is that of acn_stats_dev.h, the class comparison that of acn_surfclass.h. */
#include <hip/hip_runtime.h>
#include "acn_launch.h"
#include "acn_stats_dev.h"
#include "acn_surfclass.h"

#define SURF_PIECES  ( ACN_SURF_STRIDE / 2 )
#define STATS_PIECES ( ACN_STATS_STRIDE / 2 )
#define MOTION_PIECES ( ACN_MOTION_STRIDE / 2 )

__global__ __launch_bounds__( 256 )
void k_project_points( DevScene sc, const double* __restrict__ points, size_t n, double* __restrict__ out_pos_xy, double* __restrict__ out_depth )
{
    const size_t i = ( size_t )blockIdx.x * blockDim.x + threadIdx.x;
    if( i >= n ) return;
    const ProjCam cam = proj_cam( sc.camera_rotation, sc.prm );
    double qx, qy, ly;
    const bool projected = project_point( cam, ld3( points + 3 * i ), &qx, &qy, &ly );
    out_pos_xy[ 2 * i ] = projected ? qx : __builtin_nan( "" );
    out_pos_xy[ 2 * i + 1 ] = projected ? qy : __builtin_nan( "" );
    if( out_depth ) out_depth[ i ] = ly;
}

/* the pieces of a surface record that the rules read: { dist, pos.x } { pos.y, pos.z } { nor.x, nor.y } { nor.z, e } { x, . } and { kind, h } */
struct ReprojSurf { double2 s0, s1, s2, s3, s4, s6; };

__device__ static inline ReprojSurf reproj_surf_load( const double2* __restrict__ r )
{
    ReprojSurf s;
    s.s0 = r[ 0 ]; s.s1 = r[ 1 ]; s.s2 = r[ 2 ]; s.s3 = r[ 3 ]; s.s4 = r[ 4 ]; s.s6 = r[ 6 ];
    return s;
}

__device__ static inline SurfKey reproj_key( const ReprojSurf& s ) { return surf_key_of( s.s0.x, s.s3.y, s.s4.x, s.s6.y ); }

__device__ static inline void reproj_store( double2* out_stats, double* out_motion, size_t i, const StatsRec& t, double mx, double my )
{
    double2* o = out_stats + i * STATS_PIECES;
    #pragma unroll
    for( int k = 0; k < STATS_PIECES; k++ ) o[ k ] = t.q[ k ];
    if( out_motion ) { out_motion[ 2 * i ] = mx; out_motion[ 2 * i + 1 ] = my; }
}

/* the steps of acn_reproject* and acn_reproject_moving* for the lane's position: one body, MOVING adds step 1a and what follows from it.
 * Without MOVING motion and n_motion are not read, Pp is P, Np is N and the cap is max_history: the code of k_reproject before the table */
template< bool MOVING >
__device__ static inline void reproject_body( const double2* __restrict__ cur_surf, size_t i, const acn_params& prev, const double2* __restrict__ prev_surf,
                                              const double2* __restrict__ prev_stats, const double2* __restrict__ motion, uint64_t n_motion,
                                              const ReprojectSetup& su, double2* __restrict__ out_stats, double* __restrict__ out_motion )
{
    const double nan = __builtin_nan( "" );
    const ReprojSurf r = reproj_surf_load( cur_surf + i * SURF_PIECES );
    /* 1 HIT */
    if( !( r.s0.x < __builtin_inf() ) ) { reproj_store( out_stats, out_motion, i, stats_zero(), nan, nan ); return; }
    const V3 P = mk( r.s0.y, r.s1.x, r.s1.y ), N = mk( r.s2.x, r.s2.y, r.s3.x );
    V3 Pp = P, Np = N;
    double max_history = su.max_history;
    if constexpr( MOVING )
    {
        /* 1a OBJECT: the row of the object that carries the point; its state and its cap first, A and t only where it MOVED */
        const int32_t enter = ( int32_t )r.s3.y, id = enter >= 0 ? enter : ( int32_t )r.s4.x;
        if( id < 0 || ( uint64_t )id >= n_motion ) { reproj_store( out_stats, out_motion, i, stats_zero(), nan, nan ); return; }
        const double2* m = motion + ( size_t )id * MOTION_PIECES;
        const double2 sc = m[ 6 ];
        if( sc.x == ACN_MOTION_MOVED )
        {
            const double2 m0 = m[ 0 ], m1 = m[ 1 ], m2 = m[ 2 ], m3 = m[ 3 ], m4 = m[ 4 ], m5 = m[ 5 ];
            const V3 ax = mk( m0.x, m0.y, m1.x ), ay = mk( m1.y, m2.x, m2.y ), az = mk( m3.x, m3.y, m4.x );
            Pp = mk( v_mlv( ax, P ) + m4.y, v_mlv( ay, P ) + m5.x, v_mlv( az, P ) + m5.y );
            Np = mk( v_mlv( ax, N ), v_mlv( ay, N ), v_mlv( az, N ) );
        }
        else if( !( sc.x == ACN_MOTION_REST ) ) { reproj_store( out_stats, out_motion, i, stats_zero(), nan, nan ); return; }
        if( sc.y >= 1.0 && sc.y < max_history ) max_history = sc.y;
    }
    /* 2 MOTION */
    const ProjCam cam = proj_cam( camera_rotation_of( prev ), prev );
    double qx, qy, ly;
    if( !project_point( cam, Pp, &qx, &qy, &ly ) ) { reproj_store( out_stats, out_motion, i, stats_zero(), nan, nan ); return; }
    /* 3 ELIGIBLE */
    const uint32_t kinds = ( uint32_t )( int32_t )r.s6.x;
    const int32_t hops = ( int32_t )r.s6.y;
    if( ( kinds & su.reject_kinds ) != 0 || hops > su.max_hops ) { reproj_store( out_stats, out_motion, i, stats_zero(), qx, qy ); return; }
    /* 4 TAPS */
    const double fx = qx - 0.5, fy = qy - 0.5;
    const double x0 = __builtin_floor( fx ), y0 = __builtin_floor( fy );
    const double tx = fx - x0, ty = fy - y0;
    const double W = ( double )prev.image_width, H = ( double )prev.image_height;
    const double limit = su.plane_tolerance * r.s0.x;
    const SurfKey key = reproj_key( r );
    double sw = 0.0, sn = 0.0, smx = 0.0, smy = 0.0, smz = 0.0, s2x = 0.0, s2y = 0.0, s2z = 0.0;
    bool any = false;
    #pragma unroll
    for( int k = 0; k < 4; k++ )
    {
        const double x = ( k & 1 ) ? x0 + 1.0 : x0, y = ( k & 2 ) ? y0 + 1.0 : y0;
        const double w = ( ( k & 1 ) ? tx : 1.0 - tx ) * ( ( k & 2 ) ? ty : 1.0 - ty );
        /* 5 VALID */
        if( !( x >= 0.0 && x < W && y >= 0.0 && y < H ) || !( w > 0.0 ) ) continue;
        const size_t p = ( size_t )y * ( size_t )prev.image_width + ( size_t )x;
        const double2* tp = prev_stats + p * STATS_PIECES;
        StatsRec t;
        #pragma unroll
        for( int j = 0; j < STATS_PIECES; j++ ) t.q[ j ] = tp[ j ];
        const ReprojSurf q = reproj_surf_load( prev_surf + p * SURF_PIECES );
        if( stats_empty( t.q[ 0 ].x ) || !( q.s0.x < __builtin_inf() ) || !surf_key_eq( key, reproj_key( q ) ) ) continue;
        const V3 Nq = mk( q.s2.x, q.s2.y, q.s3.x ), D = v_sub( mk( q.s0.y, q.s1.x, q.s1.y ), Pp );
        if( !( v_mlv( Np, Nq ) >= su.normal_min ) || !( acn_fabs( v_mlv( Np, D ) ) <= limit ) ) continue;
        /* 6 GATHER */
        any = true;
        sw = sw + w;
        sn = sn + w * t.q[ 0 ].x;
        smx = smx + w * t.q[ 0 ].y; smy = smy + w * t.q[ 1 ].x; smz = smz + w * t.q[ 1 ].y;
        s2x = s2x + w * t.q[ 2 ].x; s2y = s2y + w * t.q[ 2 ].y; s2z = s2z + w * t.q[ 3 ].x;
    }
    if( !any ) { reproj_store( out_stats, out_motion, i, stats_zero(), qx, qy ); return; }
    double cnt = sn / sw, m2x = s2x / sw, m2y = s2y / sw, m2z = s2z / sw;
    if( cnt > max_history )
    {
        const double f = max_history / cnt;
        m2x = m2x * f; m2y = m2y * f; m2z = m2z * f;
        cnt = max_history;
    }
    StatsRec t;
    t.q[ 0 ] = make_double2( cnt, smx / sw ); t.q[ 1 ] = make_double2( smy / sw, smz / sw );
    t.q[ 2 ] = make_double2( m2x, m2y ); t.q[ 3 ] = make_double2( m2z, 0.0 );
    reproj_store( out_stats, out_motion, i, t, qx, qy );
}

__global__ __launch_bounds__( 256 )
void k_reproject( const double2* __restrict__ cur_surf, size_t n, acn_params prev, const double2* __restrict__ prev_surf,
                  const double2* __restrict__ prev_stats, ReprojectSetup su, double2* __restrict__ out_stats, double* __restrict__ out_motion )
{
    const size_t i = ( size_t )blockIdx.x * blockDim.x + threadIdx.x;
    if( i >= n ) return;
    reproject_body< false >( cur_surf, i, prev, prev_surf, prev_stats, nullptr, 0, su, out_stats, out_motion );
}

__global__ __launch_bounds__( 256 )
void k_reproject_moving( const double2* __restrict__ cur_surf, size_t n, acn_params prev, const double2* __restrict__ prev_surf,
                         const double2* __restrict__ prev_stats, const double2* __restrict__ motion, uint64_t n_motion, ReprojectSetup su,
                         double2* __restrict__ out_stats, double* __restrict__ out_motion )
{
    const size_t i = ( size_t )blockIdx.x * blockDim.x + threadIdx.x;
    if( i >= n ) return;
    reproject_body< true >( cur_surf, i, prev, prev_surf, prev_stats, motion, n_motion, su, out_stats, out_motion );
}

void acn_launch_project_points( const DevScene& sc, const double* points, size_t n, double* out_pos_xy, double* out_depth, hipStream_t stream )
{
    hipLaunchKernelGGL( k_project_points, dim3( ( unsigned )( ( n + 255 ) / 256 ) ), dim3( 256 ), 0, stream, sc, points, n, out_pos_xy, out_depth );
}

void acn_launch_reproject( const double* cur_surface, size_t n, const acn_params& prev, const double* prev_surface, const double* prev_stats,
                           const ReprojectSetup& su, double* out_stats, double* out_motion, hipStream_t stream )
{
    hipLaunchKernelGGL( k_reproject, dim3( ( unsigned )( ( n + 255 ) / 256 ) ), dim3( 256 ), 0, stream, ( const double2* )cur_surface, n, prev,
                        ( const double2* )prev_surface, ( const double2* )prev_stats, su, ( double2* )out_stats, out_motion );
}

void acn_launch_reproject_moving( const double* cur_surface, size_t n, const acn_params& prev, const double* prev_surface, const double* prev_stats,
                                  const double* motion, uint64_t n_motion, const ReprojectSetup& su, double* out_stats, double* out_motion,
                                  hipStream_t stream )
{
    hipLaunchKernelGGL( k_reproject_moving, dim3( ( unsigned )( ( n + 255 ) / 256 ) ), dim3( 256 ), 0, stream, ( const double2* )cur_surface, n, prev,
                        ( const double2* )prev_surface, ( const double2* )prev_stats, ( const double2* )motion, n_motion, su, ( double2* )out_stats,
                        out_motion );
}
