/* actinon_amd/csrc/acn_frame_host.h on its own, twice.  As a shared library it is the extern "C" shim through which
 * tests/test_frame_cpu.py compares the host arithmetic of the device-resident frame with tests/frame_model.py.  With
 * -DFRAME_CPU_MAIN it is a program that the same test builds with -fsanitize=address,undefined and runs: every step on heap blocks
 * of exactly their size (a read past a raster's edge is a sanitizer report), the jump against sequential steps, the draws that
 * convert to 1.0 and every refusal.  The program prints "ok" and returns 0, or names what failed. */
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "acn_frame_host.h"

static void put( const std::string& msg, char* out, size_t room )
{
    if( !out || !room ) return;
    const size_t len = msg.size() < room - 1 ? msg.size() : room - 1;
    memcpy( out, msg.data(), len );
    out[ len ] = 0;
}

extern "C"
{
uint64_t frm_jump( uint64_t v, uint64_t draws ) { return acn_frame_lcg00_jump( v, draws ); }
double frm_draw( uint64_t s ) { return acn_frame_draw_double( s ); }
void frm_key( const double* acc, uint64_t w, uint64_t h, double* key ) { acn_frame_key_host( acc, w, h, key ); }
void frm_positions( const int64_t* index, uint64_t flagged, uint64_t samples, uint64_t rval, uint64_t w, double* pos ) { acn_frame_positions_host( index, flagged, samples, rval, w, pos ); }
void frm_push( double* acc, uint64_t w, uint64_t h, const double* pos, const double* clr, uint64_t entries ) { acn_frame_push_host( acc, w, h, pos, clr, entries ); }
int64_t frm_target( double x, double y, uint64_t w, uint64_t h ) { return acn_frame_target( x, y, w, h ); }
void frm_image( const double* acc, uint64_t pixels, double* rgb, uint8_t* rgb8 ) { acn_frame_image_host( acc, pixels, rgb, rgb8 ); }
uint64_t frm_slice_groups( uint64_t slice, uint64_t samples ) { return acn_frame_slice_groups( slice, samples ); }
uint64_t frm_max_pixels( void ) { return ACN_FRAME_MAX_PIXELS; }
uint64_t frm_max_samples( void ) { return ACN_FRAME_MAX_SAMPLES; }
uint64_t frm_slice( void ) { return ACN_FRAME_SLICE; }
/* msg is written only on a refusal */
int frm_check_create( int have_handle, uint64_t w, uint64_t h, const void* out, char* msg, size_t room )
{
    std::string m; const int st = acn_frame_create_check( have_handle != 0, w, h, out, &m ); if( st != ACN_OK ) put( m, msg, room ); return st;
}
int frm_check_copy( int have_frame, const void* lum, char* msg, size_t room )
{
    std::string m; const int st = acn_frame_copy_check( have_frame != 0, lum, &m ); if( st != ACN_OK ) put( m, msg, room ); return st;
}
int frm_check_plan( int have_frame, int planned, double thr, uint64_t samples, char* msg, size_t room )
{
    std::string m; const int st = acn_frame_plan_check( have_frame != 0, planned != 0, thr, samples, &m ); if( st != ACN_OK ) put( m, msg, room ); return st;
}
int frm_check_step( int have_frame, int planned, const char* what, uint32_t world, uint64_t w, uint64_t h, uint64_t sw, uint64_t sh, int renders, char* msg, size_t room )
{
    std::string m; const int st = acn_frame_step_check( have_frame != 0, planned != 0, what, world, w, h, sw, sh, renders != 0, &m ); if( st != ACN_OK ) put( m, msg, room ); return st;
}
int frm_check_pass( int have_frame, const void* rval, char* msg, size_t room )
{
    std::string m; const int st = acn_frame_pass_check( have_frame != 0, rval, &m ); if( st != ACN_OK ) put( m, msg, room ); return st;
}
int frm_check_view( int have_frame, const void* out, char* msg, size_t room )
{
    std::string m; const int st = acn_frame_view_check( have_frame != 0, out, &m ); if( st != ACN_OK ) put( m, msg, room ); return st;
}
}

#ifdef FRAME_CPU_MAIN
static int failures = 0;
#define EXPECT( cond ) do { if( !( cond ) ) { printf( "line %d: %s\n", __LINE__, #cond ); failures++; } } while( 0 )
static bool says( const std::string& msg, const char* word ) { return msg.find( word ) != std::string::npos; }

int main()
{
    /* the jump against sequential steps */
    for( uint64_t seed : { ( uint64_t )0, ( uint64_t )21943294, ~( uint64_t )0 } )
    {
        uint64_t s = seed;
        for( uint64_t n = 0; n < 200; n++ ) { EXPECT( acn_frame_lcg00_jump( seed, n ) == s ); s = acn_frame_lcg00( s ); }
        EXPECT( acn_frame_lcg00( acn_frame_lcg00_jump( seed, ~( uint64_t )0 ) ) == seed );   /* the period is 2^64 */
        EXPECT( acn_frame_lcg00_jump( acn_frame_lcg00_jump( seed, ( uint64_t )1 << 63 ), ( uint64_t )1 << 63 ) == seed );
    }
    /* the draws at the top of the range */
    EXPECT( acn_frame_draw_double( ~( uint64_t )0 ) == 1.0 && acn_frame_draw_double( ~( uint64_t )0 - 1023 ) == 1.0 );
    EXPECT( acn_frame_draw_double( ~( uint64_t )0 - 1024 ) == 0.9999999999999999 && acn_frame_draw_double( 0 ) == 0.0 );
    EXPECT( acn_frame_draw_double( ( uint64_t )1 << 63 ) == 0.5 );

    /* every step on blocks of exactly their size: rasters with no neighbour, one row, one column, a few of each */
    const uint64_t shapes[][ 2 ] = { { 1, 1 }, { 1, 5 }, { 5, 1 }, { 7, 3 }, { 3, 7 } };
    for( const auto& sh : shapes )
    {
        const uint64_t w = sh[ 0 ], h = sh[ 1 ], n = w * h, K = 3;
        std::unique_ptr< double[] > acc( new double[ 6 * n ] ), key( new double[ n ] ), pos( new double[ 2 * n * K ] ), clr( new double[ 3 * n * K ] );
        std::unique_ptr< double[] > rgb( new double[ 3 * n ] );
        std::unique_ptr< uint8_t[] > rgb8( new uint8_t[ 3 * n ] );
        std::unique_ptr< int64_t[] > index( new int64_t[ n ] );
        for( uint64_t p = 0; p < n; p++ )
        {
            const double wgt = ( double )( p % 3 );
            const double rec[ 6 ] = { 0.5 * wgt, 0.25 * wgt, 0.1 * ( double )p, 0.7, 2.0 * wgt, wgt };
            memcpy( acc.get() + 6 * p, rec, sizeof( rec ) );
            index[ p ] = ( int64_t )p;
        }
        acn_frame_key_host( acc.get(), w, h, key.get() );
        for( uint64_t p = 0; p < n; p++ ) EXPECT( key[ p ] >= 0 );
        if( n == 1 ) EXPECT( key[ 0 ] == 0.0 );
        /* the first draw of the first entry is 2^64 - 1: its x is one past its pixel */
        const uint64_t seed = ( ~( uint64_t )0 - ACN_LCG00_C ) * 0xC097EF87329E28A5ull;   /* A^-1 mod 2^64 */
        EXPECT( acn_frame_lcg00( seed ) == ~( uint64_t )0 );
        acn_frame_positions_host( index.get(), n, K, seed, w, pos.get() );
        EXPECT( pos[ 0 ] == 1.0 );
        for( uint64_t e = 0; e < n * K; e++ ) { clr[ 3 * e ] = 0.5; clr[ 3 * e + 1 ] = 0.25; clr[ 3 * e + 2 ] = 2.0; }
        double before = 0, after = 0;
        for( uint64_t p = 0; p < n; p++ ) before += acc[ 6 * p + 5 ];
        acn_frame_push_host( acc.get(), w, h, pos.get(), clr.get(), n * K );
        for( uint64_t p = 0; p < n; p++ ) after += acc[ 6 * p + 5 ];
        uint64_t dropped = 0;
        for( uint64_t e = 0; e < n * K; e++ ) dropped += acn_frame_target( pos[ 2 * e ], pos[ 2 * e + 1 ], w, h ) < 0;
        EXPECT( after - before == ( double )( n * K - dropped ) );
        EXPECT( ( w == 1 ) == ( acn_frame_target( pos[ 0 ], pos[ 1 ], w, h ) < 0 ) );   /* one column: the entry leaves the raster */
        acn_frame_image_host( acc.get(), n, rgb.get(), rgb8.get() );
        acn_frame_image_host( acc.get(), n, nullptr, rgb8.get() );
        acn_frame_image_host( acc.get(), n, rgb.get(), nullptr );
    }
    EXPECT( acn_frame_cps( -1.0 ) == 0 && acn_frame_cps( 0.0 ) == 0 && acn_frame_cps( 1.0 ) == 255 && acn_frame_cps( 0.5 ) == 128 && acn_frame_cps( std::nan( "" ) ) == 0 );
    EXPECT( acn_frame_cps( 0.999999 ) == 255 && acn_frame_cps( 1e300 ) == 255 && acn_frame_cps( 1.0 / 256 ) == 1 );
    EXPECT( acn_frame_target( 2147483647.5, 0.5, 5, 5 ) == -1 && acn_frame_target( -0.5, 0.5, 5, 5 ) == 0 && acn_frame_target( -1.0, 0.5, 5, 5 ) == -1 );
    EXPECT( acn_frame_slice_groups( 10, 3 ) == 3 && acn_frame_slice_groups( 2, 3 ) == 1 && acn_frame_slice_groups( ACN_FRAME_SLICE, 1 ) == ACN_FRAME_SLICE );

    /* the refusals */
    std::string msg;
    int dummy = 0;
    const uint64_t big = ( uint64_t )1 << 31;
    EXPECT( acn_frame_create_check( false, 4, 4, &dummy, &msg ) == ACN_ERR_ARG && says( msg, "handle" ) );
    EXPECT( acn_frame_create_check( true, 4, 4, nullptr, &msg ) == ACN_ERR_ARG && says( msg, "out" ) );
    EXPECT( acn_frame_create_check( true, 0, 4, &dummy, &msg ) == ACN_ERR_ARG && says( msg, "width" ) );
    EXPECT( acn_frame_create_check( true, 4, 0, &dummy, &msg ) == ACN_ERR_ARG && says( msg, "height" ) );
    EXPECT( acn_frame_create_check( true, big, 1, &dummy, &msg ) == ACN_ERR_ARG && says( msg, "2^31" ) );
    EXPECT( acn_frame_create_check( true, 65536, 32769, &dummy, &msg ) == ACN_ERR_ARG && says( msg, "2^31" ) );
    EXPECT( acn_frame_create_check( true, ~( uint64_t )0, ~( uint64_t )0, &dummy, &msg ) == ACN_ERR_ARG );
    EXPECT( acn_frame_create_check( true, 65536, 32768, &dummy, &msg ) == ACN_OK && acn_frame_create_check( true, 1, 1, &dummy, &msg ) == ACN_OK );
    EXPECT( acn_frame_copy_check( false, &dummy, &msg ) == ACN_ERR_ARG && says( msg, "frame" ) );
    EXPECT( acn_frame_copy_check( true, nullptr, &msg ) == ACN_ERR_ARG && says( msg, "lum" ) );
    EXPECT( acn_frame_plan_check( false, false, 0.1, 1, &msg ) == ACN_ERR_ARG && says( msg, "frame" ) );
    EXPECT( acn_frame_plan_check( true, false, 0.1, 0, &msg ) == ACN_ERR_ARG && says( msg, "samples" ) );
    EXPECT( acn_frame_plan_check( true, false, 0.1, ACN_FRAME_MAX_SAMPLES + 1, &msg ) == ACN_ERR_ARG && says( msg, "65536" ) );
    EXPECT( acn_frame_plan_check( true, false, std::nan( "" ), 1, &msg ) == ACN_ERR_ARG && says( msg, "NaN" ) );
    EXPECT( acn_frame_plan_check( true, true, 0.1, 1, &msg ) == ACN_ERR_ARG && says( msg, "consumed" ) );
    EXPECT( acn_frame_plan_check( true, false, -INFINITY, ACN_FRAME_MAX_SAMPLES, &msg ) == ACN_OK && acn_frame_plan_check( true, false, INFINITY, 1, &msg ) == ACN_OK );
    EXPECT( acn_frame_step_check( false, true, "push", 0, 0, 0, 0, 0, false, &msg ) == ACN_ERR_ARG && says( msg, "frame" ) );
    EXPECT( acn_frame_step_check( true, false, "push", 0, 0, 0, 0, 0, false, &msg ) == ACN_ERR_ARG && says( msg, "push without a plan" ) );
    EXPECT( acn_frame_step_check( true, false, "render", 0, 4, 4, 4, 4, true, &msg ) == ACN_ERR_ARG && says( msg, "render without a plan" ) );
    EXPECT( acn_frame_step_check( true, true, "render", 2, 4, 4, 4, 4, true, &msg ) == ACN_ERR_ARG && says( msg, "sharded" ) );
    EXPECT( acn_frame_step_check( true, true, "render", 1, 4, 4, 4, 5, true, &msg ) == ACN_ERR_ARG && says( msg, "4 x 5" ) );
    EXPECT( acn_frame_step_check( true, true, "render", 1, 4, 4, 4, 4, true, &msg ) == ACN_OK && acn_frame_step_check( true, true, "push", 0, 4, 4, 9, 9, false, &msg ) == ACN_OK );
    EXPECT( acn_frame_pass_check( false, &dummy, &msg ) == ACN_ERR_ARG && says( msg, "frame" ) );
    EXPECT( acn_frame_pass_check( true, nullptr, &msg ) == ACN_ERR_ARG && says( msg, "rval" ) );
    {
        std::unique_ptr< unsigned char[] > four( new unsigned char[ 4 ] );   /* a struct_size alone, too small: nothing beyond it is read */
        const uint32_t size = 4; memcpy( four.get(), &size, 4 );
        EXPECT( acn_frame_view_check( true, four.get(), &msg ) == ACN_ERR_ARG && says( msg, "struct_size" ) );
        EXPECT( acn_frame_view_check( false, four.get(), &msg ) == ACN_ERR_ARG && says( msg, "frame" ) );
        EXPECT( acn_frame_view_check( true, nullptr, &msg ) == ACN_ERR_ARG && says( msg, "out" ) );
        acn_frame_buffers b; b.struct_size = sizeof( b );
        EXPECT( acn_frame_view_check( true, &b, &msg ) == ACN_OK );
    }

    if( failures ) { printf( "%d checks failed\n", failures ); return 1; }
    printf( "ok\n" );
    return 0;
}
#endif
