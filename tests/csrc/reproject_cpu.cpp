/* the checks of acn_reproject* in actinon_amd/csrc/acn_reproject_host.h on their own: a program that tests/test_reproject_cpu.py builds
 * with -fsanitize=address,undefined and runs.  Every refusal that needs no handle, the defaults, and parameter structs in heap blocks
 * of exactly struct_size bytes, so a read past one is a sanitizer report.  The program prints "ok" and returns 0, or names what
 * failed. */
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>

#include "acn_reproject_host.h"

static int failures = 0;
#define EXPECT( cond ) do { if( !( cond ) ) { printf( "line %d: %s\n", __LINE__, #cond ); failures++; } } while( 0 )

static bool says( const std::string& msg, const char* word ) { return msg.find( word ) != std::string::npos; }

struct Args
{
    bool handle = true;
    const void* cur; uint64_t n = 4; const acn_params* prev; const void* ps; const void* pt; const acn_reproject_params* prm = nullptr;
    const void* out; const void* motion; uint32_t world = 1;
};

static int check( const Args& a, std::string* msg, acn_reproject_params* out = nullptr )
{
    acn_reproject_params p;
    msg->clear();
    return acn_reproject_check( a.handle, a.cur, a.n, a.prev, a.ps, a.pt, a.prm, a.out, a.motion, a.world, out ? out : &p, msg );
}

/* the parameters read from a heap block of exactly `size` bytes (at least the four of struct_size itself, which every caller has) */
static int read_sized( const acn_reproject_params& src, uint32_t size, acn_reproject_params* out, std::string* msg )
{
    std::unique_ptr< char[] > block( new char[ size < 4 ? 4 : size ] );
    acn_reproject_params tmp = src;
    tmp.struct_size = size;
    memcpy( block.get(), &tmp, size < 4 ? 4 : size < sizeof( tmp ) ? size : sizeof( tmp ) );
    msg->clear();
    return acn_reproject_params_read( ( const acn_reproject_params* )block.get(), out, msg );
}

int main()
{
    std::string msg;
    alignas( 16 ) static double buf[ 512 ];
    acn_params prev = {};
    prev.image_width = 7; prev.image_height = 5;
    Args good;
    good.cur = buf; good.prev = &prev; good.ps = buf + 64; good.pt = buf + 128; good.out = buf + 192; good.motion = buf + 256;
    const double inf = std::numeric_limits< double >::infinity(), nan = std::nan( "" );

    /* the call, in the order of the header */
    acn_reproject_params got;
    EXPECT( check( good, &msg, &got ) == ACN_OK && msg.empty() );
    EXPECT( got.reject_kinds == ( ACN_SURF_CHROMATIC | ACN_SURF_FRESNEL | ACN_SURF_TRANSPARENT | ACN_SURF_CUT ) && got.max_hops == 0 );
    EXPECT( got.normal_min == 0.9 && got.plane_tolerance == 0.01 && got.max_history == 32.0 );
    { Args a = good; a.handle = false; EXPECT( check( a, &msg ) == ACN_ERR_ARG && says( msg, "handle" ) ); }
    { Args a = good; a.prev = nullptr; EXPECT( check( a, &msg ) == ACN_ERR_ARG && says( msg, "prev_params" ) ); }
    { Args a = good; a.prev = nullptr; a.n = 0; EXPECT( check( a, &msg ) == ACN_ERR_ARG && says( msg, "prev_params" ) ); }
    { Args a = good; a.cur = nullptr; EXPECT( check( a, &msg ) == ACN_ERR_ARG && says( msg, "null" ) && says( msg, "cur_surface" ) ); }
    { Args a = good; a.ps = nullptr; EXPECT( check( a, &msg ) == ACN_ERR_ARG && says( msg, "null" ) && says( msg, "prev_surface" ) ); }
    { Args a = good; a.pt = nullptr; EXPECT( check( a, &msg ) == ACN_ERR_ARG && says( msg, "null" ) && says( msg, "prev_stats" ) ); }
    { Args a = good; a.out = nullptr; EXPECT( check( a, &msg ) == ACN_ERR_ARG && says( msg, "null" ) && says( msg, "out_stats" ) ); }
    { Args a = good; a.motion = nullptr; EXPECT( check( a, &msg ) == ACN_OK ); }                                   /* the motion plane is optional */
    { Args a = good; a.cur = a.ps = a.pt = a.out = a.motion = nullptr; a.n = 0; EXPECT( check( a, &msg ) == ACN_OK ); }   /* nothing to do */
    { Args a = good; a.n = ( ( uint64_t )1 << 31 ); EXPECT( check( a, &msg ) == ACN_OK ); }
    { Args a = good; a.n = ( ( uint64_t )1 << 31 ) + 1; EXPECT( check( a, &msg ) == ACN_ERR_ARG && says( msg, "2^31" ) ); }
    { acn_params p = prev; p.image_height = 1; Args a = good; a.prev = &p; EXPECT( check( a, &msg ) == ACN_ERR_ARG && says( msg, "raster" ) ); }
    { acn_params p = prev; p.image_width = 0; Args a = good; a.prev = &p; EXPECT( check( a, &msg ) == ACN_ERR_ARG && says( msg, "raster" ) ); }
    { acn_params p = prev; p.image_width = 1u << 16; p.image_height = 1u << 15; Args a = good; a.prev = &p; EXPECT( check( a, &msg ) == ACN_OK ); }
    { acn_params p = prev; p.image_width = 1u << 16; p.image_height = ( 1u << 15 ) + 1; Args a = good; a.prev = &p; EXPECT( check( a, &msg ) == ACN_ERR_ARG && says( msg, "2^31" ) ); }
    { acn_params p = prev; p.image_width = ( uint64_t )1 << 33; p.image_height = ( uint64_t )1 << 33; Args a = good; a.prev = &p; EXPECT( check( a, &msg ) == ACN_ERR_ARG && says( msg, "2^31" ) ); }   /* (the product wraps to 4) */
    for( int which = 0; which < 4; which++ )
    {
        Args a = good;
        ( which == 0 ? a.cur : which == 1 ? a.ps : which == 2 ? a.pt : a.out ) = ( const char* )buf + 8 + which * 512;
        EXPECT( check( a, &msg ) == ACN_ERR_ARG && says( msg, "align" ) );
    }
    { Args a = good; a.motion = ( const char* )a.motion + 8; EXPECT( check( a, &msg ) == ACN_OK ); }                /* an array of doubles */
    { Args a = good; a.motion = ( const char* )a.motion + 4; EXPECT( check( a, &msg ) == ACN_ERR_ARG && says( msg, "out_motion" ) ); }
    { Args a = good; a.world = 2; EXPECT( check( a, &msg ) == ACN_ERR_ARG && says( msg, "sharded" ) ); }
    { Args a = good; a.world = 0; EXPECT( check( a, &msg ) == ACN_OK ); }

    /* the parameters */
    const acn_reproject_params init = ACN_REPROJECT_PARAMS_INIT;
    EXPECT( init.struct_size == sizeof( acn_reproject_params ) && sizeof( acn_reproject_params ) == 40 );
    auto with = [ & ]( acn_reproject_params p ) { Args a = good; a.prm = &p; return check( a, &msg, &got ); };
    EXPECT( with( init ) == ACN_OK && got.normal_min == 0.9 && got.max_history == 32.0 );
    for( uint32_t size = 0; size < 4; size++ ) EXPECT( read_sized( init, size, &got, &msg ) == ACN_ERR_ARG && says( msg, "struct_size" ) );
    { acn_reproject_params p = init; p.flags = 4u; EXPECT( with( p ) == ACN_ERR_ARG && says( msg, "flags" ) ); }
    { acn_reproject_params p = init; p.flags = ACN_REPROJECT_KINDS_SET; EXPECT( with( p ) == ACN_OK && got.reject_kinds == 0 ); }
    { acn_reproject_params p = init; p.reject_kinds = ACN_SURF_EMITTER; EXPECT( with( p ) == ACN_OK && got.reject_kinds == ACN_SURF_EMITTER ); }
    { acn_reproject_params p = init; p.flags = ACN_REPROJECT_HOPS_SET; p.max_hops = 3; EXPECT( with( p ) == ACN_OK && got.max_hops == 3 ); }
    { acn_reproject_params p = init; p.max_hops = 2; EXPECT( with( p ) == ACN_OK && got.max_hops == 2 ); }
    { acn_reproject_params p = init; p.normal_min = -1.0; EXPECT( with( p ) == ACN_OK && got.normal_min == -1.0 ); }
    { acn_reproject_params p = init; p.normal_min = 1.0; EXPECT( with( p ) == ACN_OK && got.normal_min == 1.0 ); }
    for( double v : { -1.0000001, 1.0000001, inf, -inf, nan } ) { acn_reproject_params p = init; p.normal_min = v; EXPECT( with( p ) == ACN_ERR_ARG && says( msg, "normal_min" ) ); }
    for( double v : { -1e-300, -1.0, inf, -inf, nan } ) { acn_reproject_params p = init; p.plane_tolerance = v; EXPECT( with( p ) == ACN_ERR_ARG && says( msg, "plane_tolerance" ) ); }
    { acn_reproject_params p = init; p.plane_tolerance = 1e300; EXPECT( with( p ) == ACN_OK && got.plane_tolerance == 1e300 ); }
    for( double v : { 0.5, -1.0, 0.9999999, inf, -inf, nan } ) { acn_reproject_params p = init; p.max_history = v; EXPECT( with( p ) == ACN_ERR_ARG && says( msg, "max_history" ) ); }
    { acn_reproject_params p = init; p.max_history = 1.0; EXPECT( with( p ) == ACN_OK && got.max_history == 1.0 ); }
    { acn_reproject_params p = init; p.max_history = 2.5; EXPECT( with( p ) == ACN_OK && got.max_history == 2.5 ); }

    /* a caller compiled against a shorter struct: members it does not reach take their defaults, and nothing beyond its size is read */
    acn_reproject_params full = init;
    full.flags = ACN_REPROJECT_KINDS_SET; full.reject_kinds = ACN_SURF_EMITTER; full.max_hops = 1; full.normal_min = 0.5; full.plane_tolerance = 0.25; full.max_history = 4.0;
    EXPECT( read_sized( full, 4, &got, &msg ) == ACN_OK && got.reject_kinds == ACN_REPROJECT_DEFAULT_REJECT_KINDS && got.max_hops == 0 && got.normal_min == 0.9 );
    EXPECT( read_sized( full, 8, &got, &msg ) == ACN_OK && got.reject_kinds == 0 && got.max_hops == 0 );              /* the flag without the member: no kind is rejected */
    EXPECT( read_sized( full, 16, &got, &msg ) == ACN_OK && got.reject_kinds == ACN_SURF_EMITTER && got.max_hops == 1 && got.normal_min == 0.9 && got.max_history == 32.0 );
    EXPECT( read_sized( full, 24, &got, &msg ) == ACN_OK && got.normal_min == 0.5 && got.plane_tolerance == 0.01 );
    EXPECT( read_sized( full, 32, &got, &msg ) == ACN_OK && got.plane_tolerance == 0.25 && got.max_history == 32.0 );
    EXPECT( read_sized( full, 40, &got, &msg ) == ACN_OK && got.max_history == 4.0 );
    EXPECT( read_sized( full, 4096, &got, &msg ) == ACN_OK && got.max_history == 4.0 );                                 /* a longer struct of a later header */
    EXPECT( acn_reproject_params_read( nullptr, &got, &msg ) == ACN_OK && got.normal_min == 0.9 && got.reject_kinds == ACN_REPROJECT_DEFAULT_REJECT_KINDS );

    if( failures ) { printf( "%d checks failed\n", failures ); return 1; }
    printf( "ok\n" );
    return 0;
}
