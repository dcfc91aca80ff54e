/* acn_dev_base.h -- the bottom layer of the device code (acn_device.h lists the layers): the inlining macros, the constants of
 * vectors.h, V3 / M3, the address spaces the scene is read through, the vector functions and the LCGs with the sampling built on
 * them.  Of a scene it knows the record types the typedefs point to (acn_tables.h) and nothing else. */
#ifndef ACN_DEV_BASE_H
#define ACN_DEV_BASE_H

#include <hip/hip_runtime.h>
#include "actinon_hip.h"
#include "acn_tables.h"   /* GNode, GMat, SCEntry, the flag / opcode constants and the depth and LDS limits: shared with the host-only table builder */
#include "acn_detmath.h"

#pragma clang fp contract(off)

#define DEV __device__ __forceinline__
#define DEVN __device__ __noinline__

#define F3_INF ( __builtin_huge_val() )
#define F3_MAG 1E+30
#define F3_EPS 1E-6
#define ACN_PI 3.14159265358979323846

struct V3 { double x, y, z; };
struct M3 { V3 x, y, z; };

/* The scene arrays are read through the CONSTANT address space: they never change while a kernel runs, so a load
 * whose address is the same in every lane (root-compound loops, a wave's shading task) is issued as a scalar load
 * (s_load -> SGPRs, scalar cache) and costs neither vector-memory bandwidth nor VGPRs; loads with per-lane
 * addresses (inside CSG trees) become ordinary global loads. */
#define ACN_CONST __attribute__( ( address_space( 4 ) ) )
typedef const GNode   ACN_CONST* NodeP;
typedef const GMat    ACN_CONST* MatP;
typedef const int32_t ACN_CONST* ElemP;
typedef const acn_texture ACN_CONST* TexP;

/* node array staged in LDS (per workgroup) for the kernels whose node accesses are per-lane */
#define ACN_LDS __attribute__( ( address_space( 3 ) ) )
typedef const GNode ACN_LDS* LdsNodeP;
typedef double ACN_LDS* LdsF64P;
typedef uint32_t ACN_LDS* LdsU32P;

/* ---- vectors.h ---- */
DEV V3 mk( double x, double y, double z ) { V3 v; v.x = x; v.y = y; v.z = z; return v; }
template< class P > DEV V3 ld3( P p ) { return mk( p[ 0 ], p[ 1 ], p[ 2 ] ); }
DEV V3 ldc( const V3 ACN_CONST& v ) { return mk( v.x, v.y, v.z ); }
DEV V3 v_neg( V3 o ) { return mk( -o.x, -o.y, -o.z ); }
DEV double v_sqr( V3 o ) { return ( o.x * o.x ) + ( o.y * o.y ) + ( o.z * o.z ); }
DEV V3 v_add( V3 o, V3 s ) { return mk( o.x + s.x, o.y + s.y, o.z + s.z ); }
DEV V3 v_sub( V3 o, V3 s ) { return mk( o.x - s.x, o.y - s.y, o.z - s.z ); }
DEV V3 v_mlf( V3 o, double f ) { return mk( o.x * f, o.y * f, o.z * f ); }
DEV V3 v_mlx( V3 o, V3 f ) { return mk( o.y * f.z - o.z * f.y, o.z * f.x - o.x * f.z, o.x * f.y - o.y * f.x ); }
DEV V3 v_mld( V3 o, V3 f ) { return mk( o.x * f.x, o.y * f.y, o.z * f.z ); }
DEV double v_mlv( V3 o, V3 m ) { return ( o.x * m.x ) + ( o.y * m.y ) + ( o.z * m.z ); }
DEV double v_sub_mlv( V3 o, V3 s, V3 m ) { return ( ( o.x - s.x ) * m.x ) + ( ( o.y - s.y ) * m.y ) + ( ( o.z - s.z ) * m.z ); }
DEV double f_sqr( double a ) { return a * a; }
DEV double v_diff_sqr( V3 o, V3 v ) { return f_sqr( o.x - v.x ) + f_sqr( o.y - v.y ) + f_sqr( o.z - v.z ); }
DEV double f_max( double a, double b ) { return a > b ? a : b; }
DEV double f_min( double a, double b ) { return a < b ? a : b; }
DEV double f_abs( double a ) { return a < 0 ? -a : a; }

DEV V3 v_of_length( V3 o, double a )   /* vectors.h:148-154 */
{
    double r_sqr = v_sqr( o );
    if( acn_fabs( r_sqr - 1.0 ) < 1E-8 ) return o;
    double f = r_sqr > 0 ? ( a / acn_sqrt( r_sqr ) ) : 0;
    return mk( o.x * f, o.y * f, o.z * f );
}

DEV V3 v_von( V3 o, V3 v )   /* vectors.h:157-162 */
{
    V3 o_n = v_of_length( o, 1.0 );
    v = v_sub( v, v_mlf( o_n, v_mlv( o_n, v ) ) );
    return v_of_length( v, 1.0 );
}

DEV V3 v_con( V3 o )   /* vectors.h:165-175 */
{
    double xx = o.x * o.x;
    double yy = o.y * o.y;
    double zz = o.z * o.z;
    V3 v;
    v.x = ( ( xx <= yy ) && ( xx <= zz ) ) ? 1 : 0;
    v.y = ( ( yy <= xx ) && ( yy <= zz ) ) ? 1 : 0;
    v.z = ( ( zz <= xx ) && ( zz <= yy ) ) ? 1 : 0;
    return v_von( o, v );
}

DEV V3 m_mlv( const M3& o, V3 v )   /* vectors.h:256-265 */
{
    return mk( o.x.x * v.x + o.x.y * v.y + o.x.z * v.z,
               o.y.x * v.x + o.y.y * v.y + o.y.z * v.z,
               o.z.x * v.x + o.z.y * v.y + o.z.z * v.z );
}

DEV V3 m_tmlv( const M3& o, V3 v )   /* vectors.h:268-276 */
{
    return mk( o.x.x * v.x + o.y.x * v.y + o.z.x * v.z,
               o.x.y * v.x + o.y.y * v.y + o.z.y * v.z,
               o.x.z * v.x + o.y.z * v.y + o.z.z * v.z );
}

DEV M3 m_transposed( const M3& o )
{
    M3 r;
    r.x = mk( o.x.x, o.y.x, o.z.x );
    r.y = mk( o.x.y, o.y.y, o.z.y );
    r.z = mk( o.x.z, o.y.z, o.z.z );
    return r;
}

DEV M3 m_con_z( V3 v )   /* vectors.h:315-322 */
{
    M3 m;
    m.z = v_of_length( v, 1.0 );
    m.x = v_con( v );
    m.y = v_mlx( m.z, m.x );
    return m;
}

DEV V3 ray_pos( V3 p, V3 d, double offs ) { return v_add( p, v_mlf( d, offs ) ); }   /* vectors.h:343-346 */

DEV V3 v_orthogonal_projection( V3 o, V3 nor )   /* vectors.h:223-232 */
{
    double f = v_mlv( o, nor );
    return mk( o.x - nor.x * f, o.y - nor.y * f, o.z - nor.z * f );
}

DEV V3 v_reflection( V3 dir, V3 nor )   /* vectors.h:238-241 */
{
    return v_of_length( v_sub( dir, v_mlf( nor, 2.0 * v_mlv( dir, nor ) ) ), 1.0 );
}

/* ---- LCG / sampling: vectors.h:45-48, 177-206 ---- */
DEV uint64_t lcg00( uint64_t v ) { return v * ACN_LCG00_A + ACN_LCG00_C; }
DEV uint64_t lcg01( uint64_t v ) { return v * ACN_LCG01_A + ACN_LCG01_C; }
DEV uint64_t lcg02( uint64_t v ) { return v * ACN_LCG02_A + ACN_LCG02_C; }
DEV double f3_rnd0( uint64_t* rv ) { return ( double )( *rv = lcg00( *rv ) ) * ( 2.0 / 0xFFFFFFFFFFFFFFFFull ) - 1.0; }
DEV double f3_rnd1( uint64_t* rv ) { return ( double )( *rv = lcg00( *rv ) ) * ( 1.0 / 0xFFFFFFFFFFFFFFFFull ); }

/* advance an lcg00 state by k steps in O(log k) (Brown's arbitrary-stride formula) */
DEV uint64_t lcg00_jump( uint64_t v, uint64_t k )
{
    uint64_t a = ACN_LCG00_A, c = ACN_LCG00_C;
    uint64_t acc_a = 1, acc_c = 0;
    while( k )
    {
        if( k & 1 ) { acc_a *= a; acc_c = acc_c * a + c; }
        c = ( a + 1 ) * c;
        a *= a;
        k >>= 1;
    }
    return acc_a * v + acc_c;
}

DEV uint64_t seed_from_f3( double v )
{
    int64_t seed_s3 = ( int64_t )( acn_frexp_mant( v ) * ( double )0x7FFFFFFFFFFFFFFF );
    return ( uint64_t )seed_s3 * 27362149ull;
}

DEV uint64_t v_random_seed( V3 o, uint64_t rv )
{
    return seed_from_f3( o.x ) * lcg00( rv ) + seed_from_f3( o.y ) * lcg01( rv ) + seed_from_f3( o.z ) * lcg02( rv );
}

DEV V3 v_random_sphere_cap( uint64_t* rv, double h )
{
    V3 v;
    double phi = 2.0 * ACN_PI * f3_rnd1( rv );
    v.z = 1.0 - f3_rnd1( rv ) * h;
    double scale = acn_sqrt( 1.0 - v.z * v.z );
    double s, c;
    acn_sincos( phi, &s, &c );
    v.x = s * scale;
    v.y = c * scale;
    return v;
}

DEV V3 v_random_sphere_belt( uint64_t* rv, double h )   /* vectors.h:209-218 */
{
    V3 v;
    double phi = 2.0 * ACN_PI * f3_rnd1( rv );
    v.z = f3_rnd0( rv ) * h;
    double scale = acn_sqrt( 1.0 - v.z * v.z );
    double s, c;
    acn_sincos( phi, &s, &c );
    v.x = s * scale;
    v.y = c * scale;
    return v;
}

#endif /* ACN_DEV_BASE_H */
