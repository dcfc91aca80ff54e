/* acn_frame_host.h -- the arithmetic of a device-resident frame (include/actinon_hip.h, acn_frame_*) as one expression per step
 * for host and device, and every argument check of the frame calls with its message.  Plain C++, no HIP header: k_frame.hip
 * compiles the step functions for the device, acn_calls.hip runs the checks before it touches a handle, and tests/csrc/frame_cpu.cpp
 * compiles the header on its own, as a shim for the CPU tests and as a program that runs under the address and undefined-behaviour
 * sanitizers.  Each step is the render driver's (actinon_amd/host/acn_driver.c), in its evaluation order; tests/frame_model.py
 * restates them in numpy. */
#ifndef ACN_FRAME_HOST_H
#define ACN_FRAME_HOST_H

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>

#include "actinon_hip.h"

#if defined( __HIPCC__ )
#define ACN_FRAME_HD __host__ __device__
#else
#define ACN_FRAME_HD
#endif

/* a raster has at most 2^31 pixels and fewer than 2^31 columns and rows: ( int32_t )pos of a position inside it, and of the
 * position one past its last column or row, is defined */
#define ACN_FRAME_MAX_PIXELS ( ( uint64_t )1 << 31 )
#define ACN_FRAME_MAX_SAMPLES ( ( uint64_t )1 << 16 )
/* positions of one slice of a pass (the handle's tunable ACN_FRAME_SLICE lowers it: tests) */
#define ACN_FRAME_SLICE ( ( uint64_t )1 << 24 )
/* foreign entries of a pass that push keeps in a list; beyond that one lane walks the whole plan */
#define ACN_FRAME_FOREIGN_SLOTS 1024u

/* an lcg00 state advanced by `draws` steps in O( log draws ): the loop of lcg00_jump (acn_device.h) */
ACN_FRAME_HD static inline uint64_t acn_frame_lcg00_jump( uint64_t v, uint64_t draws )
{
    uint64_t a = ACN_LCG00_A, c = ACN_LCG00_C;
    uint64_t acc_a = 1, acc_c = 0;
    while( draws )
    {
        if( draws & 1 ) { acc_a *= a; acc_c = acc_c * a + c; }
        c = ( a + 1 ) * c;
        a *= a;
        draws >>= 1;
    }
    return acc_a * v + acc_c;
}

ACN_FRAME_HD static inline uint64_t acn_frame_lcg00( uint64_t v ) { return v * ACN_LCG00_A + ACN_LCG00_C; }

/* f3_rnd1 of a draw: the constant is 2^-64, a draw of 2^64 - 1024 or more gives exactly 1.0 */
ACN_FRAME_HD static inline double acn_frame_draw_double( uint64_t s ) { return ( double )s * ( 1.0 / 0xFFFFFFFFFFFFFFFFull ); }

/* entry e = r * K + k of a plan: the position in pixel ( i, j ) = the r-th flagged one */
ACN_FRAME_HD static inline void acn_frame_position( uint64_t rval, uint64_t e, uint64_t i, uint64_t j, double* pos_xy )
{
    const uint64_t s = acn_frame_lcg00_jump( rval, 2 * e );
    const uint64_t s1 = acn_frame_lcg00( s ), s2 = acn_frame_lcg00( s1 );
    pos_xy[ 0 ] = ( double )( int64_t )i + acn_frame_draw_double( s1 );
    pos_xy[ 1 ] = ( double )( int64_t )j + acn_frame_draw_double( s2 );
}

/* lum_image_avg_clr of a record ( pos_x pos_y clr[ 3 ] weight ) */
ACN_FRAME_HD static inline void acn_frame_avg( const double* rec, double* avg )
{
    const double f = ( rec[ 5 ] > 0 ) ? 1.0 / rec[ 5 ] : 1.0;
    avg[ 0 ] = rec[ 2 ] * f; avg[ 1 ] = rec[ 3 ] * f; avg[ 2 ] = rec[ 4 ] * f;
}

/* lum_image_clr_dev of a neighbour inside the raster, and the step of lum_image_sqr_grad's maximum */
ACN_FRAME_HD static inline double acn_frame_clr_dev( const double* ref, const double* c )
{
    const double dx = ref[ 0 ] - c[ 0 ], dy = ref[ 1 ] - c[ 1 ], dz = ref[ 2 ] - c[ 2 ];
    return ( dx * dx ) + ( dy * dy ) + ( dz * dz );
}
ACN_FRAME_HD static inline double acn_frame_grad_max( double g0, double g1 ) { return g1 > g0 ? g1 : g0; }

/* the eight neighbours in the driver's order */
#define ACN_FRAME_NEIGHBOURS 8
#define ACN_FRAME_NB_DX( k ) ( ( k ) < 3 ? -1 : ( k ) < 5 ? 0 : 1 )
#define ACN_FRAME_NB_DY( k ) ( ( k ) < 3 ? ( k ) - 1 : ( k ) == 3 ? -1 : ( k ) == 4 ? 1 : ( k ) - 6 )

/* lum_image_push: the pixel an entry lands in, -1 outside the raster */
ACN_FRAME_HD static inline int64_t acn_frame_target( double pos_x, double pos_y, uint64_t width, uint64_t height )
{
    const int32_t x = ( int32_t )pos_x, y = ( int32_t )pos_y;
    if( x >= 0 && ( uint64_t )x < width && y >= 0 && ( uint64_t )y < height ) return ( int64_t )( ( uint64_t )y * width + ( uint64_t )x );
    return -1;
}

/* ... and what it adds to the record, weight 1, in the order of the array */
ACN_FRAME_HD static inline void acn_frame_add( double* rec, double pos_x, double pos_y, const double* clr )
{
    rec[ 0 ] += pos_x; rec[ 1 ] += pos_y;
    rec[ 2 ] += clr[ 0 ]; rec[ 3 ] += clr[ 1 ]; rec[ 4 ] += clr[ 2 ];
    rec[ 5 ] += 1.0;
}

/* a channel of acn_cps_from_cl */
ACN_FRAME_HD static inline uint8_t acn_frame_cps( double c ) { return c > 0.0 ? c < 1.0 ? ( uint8_t )( c * 256 ) : 255 : 0; }

/* ---- whole steps on host arrays: what the kernels are compared with ---- */
static inline void acn_frame_key_host( const double* acc, uint64_t width, uint64_t height, double* key )
{
    for( uint64_t y = 0; y < height; y++ ) for( uint64_t x = 0; x < width; x++ )
    {
        double v[ 3 ], c[ 3 ], g0 = 0;
        acn_frame_avg( acc + 6 * ( y * width + x ), v );
        for( int k = 0; k < ACN_FRAME_NEIGHBOURS; k++ )
        {
            const int64_t nx = ( int64_t )x + ACN_FRAME_NB_DX( k ), ny = ( int64_t )y + ACN_FRAME_NB_DY( k );
            double g1 = 0;
            if( nx >= 0 && ( uint64_t )nx < width && ny >= 0 && ( uint64_t )ny < height )
            {
                acn_frame_avg( acc + 6 * ( ( uint64_t )ny * width + ( uint64_t )nx ), c );
                g1 = acn_frame_clr_dev( v, c );
            }
            g0 = acn_frame_grad_max( g0, g1 );
        }
        key[ y * width + x ] = g0;
    }
}

static inline void acn_frame_positions_host( const int64_t* index, uint64_t flagged, uint64_t samples, uint64_t rval, uint64_t width, double* pos_xy )
{
    for( uint64_t r = 0; r < flagged; r++ ) for( uint64_t k = 0; k < samples; k++ )
    {
        const uint64_t p = ( uint64_t )index[ r ], e = r * samples + k;
        acn_frame_position( rval, e, p % width, p / width, pos_xy + 2 * e );
    }
}

/* the driver's loop: every entry in the order of the array */
static inline void acn_frame_push_host( double* acc, uint64_t width, uint64_t height, const double* pos_xy, const double* clr, uint64_t entries )
{
    for( uint64_t e = 0; e < entries; e++ )
    {
        const int64_t t = acn_frame_target( pos_xy[ 2 * e ], pos_xy[ 2 * e + 1 ], width, height );
        if( t >= 0 ) acn_frame_add( acc + 6 * t, pos_xy[ 2 * e ], pos_xy[ 2 * e + 1 ], clr + 3 * e );
    }
}

static inline void acn_frame_image_host( const double* acc, uint64_t pixels, double* rgb, uint8_t* rgb8 )
{
    for( uint64_t p = 0; p < pixels; p++ )
    {
        double avg[ 3 ];
        acn_frame_avg( acc + 6 * p, avg );
        for( int c = 0; c < 3; c++ )
        {
            if( rgb ) rgb[ 3 * p + c ] = avg[ c ];
            if( rgb8 ) rgb8[ 3 * p + c ] = acn_frame_cps( avg[ c ] );
        }
    }
}

/* groups of one slice of a pass with `samples` entries per group: whole groups, at least one */
static inline uint64_t acn_frame_slice_groups( uint64_t slice_positions, uint64_t samples )
{
    const uint64_t g = slice_positions / samples;
    return g ? g : 1;
}

/* ---- the argument checks, on the host before anything is written; on a refusal *msg is what acn_last_error will carry ---- */
static inline int acn_frame_create_check( bool have_handle, uint64_t width, uint64_t height, const void* out, std::string* msg )
{
    if( !have_handle ) { *msg = "null argument: handle"; return ACN_ERR_ARG; }
    if( !out ) { *msg = "null argument: out"; return ACN_ERR_ARG; }
    if( width == 0 || height == 0 ) { *msg = "a frame needs a width and a height"; return ACN_ERR_ARG; }
    if( width >= ACN_FRAME_MAX_PIXELS || height >= ACN_FRAME_MAX_PIXELS || width * height > ACN_FRAME_MAX_PIXELS )
    {
        *msg = "a frame has at most 2^31 pixels and fewer than 2^31 columns and rows";
        return ACN_ERR_ARG;
    }
    return ACN_OK;
}

/* upload, download: the frame and the host array */
static inline int acn_frame_copy_check( bool have_frame, const void* lum, std::string* msg )
{
    if( !have_frame ) { *msg = "null argument: frame"; return ACN_ERR_ARG; }
    if( !lum ) { *msg = "null argument: lum"; return ACN_ERR_ARG; }
    return ACN_OK;
}

/* planned: the frame holds a plan that no push has consumed */
static inline int acn_frame_plan_check( bool have_frame, bool planned, double sqr_threshold, uint64_t samples, std::string* msg )
{
    if( !have_frame ) { *msg = "null argument: frame"; return ACN_ERR_ARG; }
    if( samples == 0 ) { *msg = "samples is 0"; return ACN_ERR_ARG; }
    if( samples > ACN_FRAME_MAX_SAMPLES ) { *msg = "samples " + std::to_string( samples ) + " is above 65536"; return ACN_ERR_ARG; }
    if( sqr_threshold != sqr_threshold ) { *msg = "sqr_threshold is NaN"; return ACN_ERR_ARG; }
    if( planned ) { *msg = "the frame holds a plan that no push has consumed"; return ACN_ERR_ARG; }
    return ACN_OK;
}

/* render ( what = "render" ) and push ( "push" ): they need a plan; render also the scene's raster */
static inline int acn_frame_step_check( bool have_frame, bool planned, const char* what, uint32_t shard_world, uint64_t width, uint64_t height,
                                        uint64_t scene_width, uint64_t scene_height, bool renders, std::string* msg )
{
    if( !have_frame ) { *msg = "null argument: frame"; return ACN_ERR_ARG; }
    if( shard_world > 1 ) { *msg = "a frame call is not sharded"; return ACN_ERR_ARG; }
    if( !planned ) { *msg = std::string( what ) + " without a plan: acn_frame_plan comes first"; return ACN_ERR_ARG; }
    if( renders && ( width != scene_width || height != scene_height ) )
    {
        *msg = "the frame is " + std::to_string( width ) + " x " + std::to_string( height ) + ", the raster of the resident scene " +
               std::to_string( scene_width ) + " x " + std::to_string( scene_height );
        return ACN_ERR_ARG;
    }
    return ACN_OK;
}

static inline int acn_frame_pass_check( bool have_frame, const void* rval, std::string* msg )
{
    if( !have_frame ) { *msg = "null argument: frame"; return ACN_ERR_ARG; }
    if( !rval ) { *msg = "null argument: rval"; return ACN_ERR_ARG; }
    return ACN_OK;
}

static inline int acn_frame_view_check( bool have_frame, const void* out, std::string* msg )
{
    if( !have_frame ) { *msg = "null argument: frame"; return ACN_ERR_ARG; }
    if( !out ) { *msg = "null argument: out"; return ACN_ERR_ARG; }
    uint32_t size;
    memcpy( &size, out, sizeof( size ) );
    if( size < 8 ) { *msg = "acn_frame_buffers.struct_size " + std::to_string( size ) + " is smaller than its first members (8 bytes)"; return ACN_ERR_ARG; }
    return ACN_OK;
}

#endif
