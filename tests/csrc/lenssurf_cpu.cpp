/* actinon_amd/csrc/acn_lenssurf_host.h on its own: a program that tests/test_lens_surface_cpu.py builds with
 * -fsanitize=address,undefined and runs.  Every refusal of acn_surface_reduce* and acn_surface_lens* that needs no handle, with each
 * acn_lens_params in a heap block of exactly its struct_size, so a read past a short one is a sanitizer report; and the slice
 * arithmetic.  The program prints "ok" and returns 0, or names what failed. */
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <memory>

#include "acn_lenssurf_host.h"

static int failures = 0;
#define EXPECT( cond ) do { if( !( cond ) ) { printf( "line %d: %s\n", __LINE__, #cond ); failures++; } } while( 0 )

static bool says( const std::string& msg, const char* word ) { return msg.find( word ) != std::string::npos; }

/* the lens check with the first `bytes` bytes of p in a heap block of that size */
static int lens( const acn_lens_params& p, size_t bytes, bool need_pos, const void* pos, uint64_t n, uint32_t mode, const void* out, uint32_t world,
                 acn_lens_params* read, std::string* msg, bool have_handle = true )
{
    std::unique_ptr< unsigned char[] > block( new unsigned char[ bytes ] );
    memcpy( block.get(), &p, bytes );
    msg->clear();
    return acn_lenssurf_lens_check( have_handle, need_pos, pos, n, ( const acn_lens_params* )block.get(), mode, out, world, read, msg );
}

static int reduce( bool have_handle, const void* rec, uint64_t n, uint32_t K, const void* out, uint32_t world, std::string* msg )
{
    msg->clear();
    return acn_lenssurf_reduce_check( have_handle, rec, n, K, out, world, msg );
}

int main()
{
    std::string msg;
    const double inf = std::numeric_limits< double >::infinity(), nan = std::nan( "" );
    alignas( 16 ) static double buf[ 64 ];
    const void* in = buf; const void* out = buf + 32;

    /* the reduce calls, in the order of the header */
    EXPECT( reduce( true, in, 4, 16, out, 1, &msg ) == ACN_OK && msg.empty() );
    EXPECT( reduce( false, in, 4, 16, out, 1, &msg ) == ACN_ERR_ARG && says( msg, "handle" ) );
    EXPECT( reduce( true, nullptr, 4, 16, out, 1, &msg ) == ACN_ERR_ARG && says( msg, "null" ) && says( msg, "records" ) );
    EXPECT( reduce( true, in, 4, 16, nullptr, 1, &msg ) == ACN_ERR_ARG && says( msg, "null" ) && says( msg, "out" ) );
    EXPECT( reduce( true, nullptr, 0, 16, nullptr, 0, &msg ) == ACN_OK );
    EXPECT( reduce( true, in, 4, 0, out, 1, &msg ) == ACN_ERR_ARG && says( msg, "K 0" ) );
    EXPECT( reduce( true, nullptr, 0, 0, nullptr, 1, &msg ) == ACN_ERR_ARG && says( msg, "K 0" ) );     /* (also with nothing to do) */
    EXPECT( reduce( true, in, 4, 4097, out, 1, &msg ) == ACN_ERR_ARG && says( msg, "4097" ) );
    EXPECT( reduce( true, in, 4, 0xFFFFFFFFu, out, 1, &msg ) == ACN_ERR_ARG );
    EXPECT( reduce( true, in, 4, 1, out, 1, &msg ) == ACN_OK && reduce( true, in, 4, 4096, out, 1, &msg ) == ACN_OK );
    EXPECT( reduce( true, in, 4, 16, out, 2, &msg ) == ACN_ERR_ARG && says( msg, "sharded" ) );
    EXPECT( reduce( true, ( const char* )in + 8, 4, 16, out, 1, &msg ) == ACN_ERR_ARG && says( msg, "align" ) );
    EXPECT( reduce( true, in, 4, 16, ( const char* )out + 8, 1, &msg ) == ACN_ERR_ARG && says( msg, "align" ) );
    EXPECT( reduce( true, in, 4, 16, ( const char* )out + 1, 1, &msg ) == ACN_ERR_ARG && says( msg, "align" ) );
    EXPECT( reduce( true, in, ( ( uint64_t )1 << 38 ) + 1, 16, out, 1, &msg ) == ACN_ERR_ARG && says( msg, "2^38" ) );
    EXPECT( reduce( true, in, ( uint64_t )1 << 38, 16, out, 1, &msg ) == ACN_OK );

    /* the lens calls: every layout a caller may have been compiled with */
    acn_lens_params p = ACN_LENS_PARAMS_INIT, read;
    p.samples = 8; p.flags = ACN_LENS_JITTER; p.seed = 5; p.aperture_radius = 0.25; p.focus_distance = 12.0;
    for( uint32_t size = 0; size <= sizeof( p ) + 8; size++ )
    {
        acn_lens_params q = p;
        q.struct_size = size;
        const size_t have = size < sizeof( q ) ? ( size < 4 ? 4 : size ) : sizeof( q );
        const int st = lens( q, have, true, in, 4, ACN_SURF_FOLLOW, out, 1, &read, &msg );
        if( size < 4 ) { EXPECT( st == ACN_ERR_ARG && says( msg, "struct_size" ) ); continue; }
        if( size % 4 || ( size > 16 && size % 8 ) ) continue;   /* (a size inside a member: part of its bytes) */
        if( size >= 24 && size < 32 ) { EXPECT( st == ACN_ERR_ARG && says( msg, "focus" ) ); continue; }   /* an aperture without its focus */
        EXPECT( st == ACN_OK );
        EXPECT( read.samples == ( size >= 8 ? 8u : 0u ) && read.flags == ( size >= 12 ? ACN_LENS_JITTER : 0u ) && read.seed == ( size >= 16 ? 5u : 0u ) );
        EXPECT( read.aperture_radius == ( size >= 24 ? 0.25 : 0.0 ) && read.focus_distance == ( size >= 32 ? 12.0 : 0.0 ) );
    }
    msg.clear();
    EXPECT( acn_lenssurf_lens_check( true, true, in, 4, nullptr, ACN_SURF_FIRST_HIT, out, 1, &read, &msg ) == ACN_OK && read.samples == 0 && read.aperture_radius == 0.0 );
    /* the refusals, in the order of the header */
    const size_t all = sizeof( p );
    EXPECT( lens( p, all, true, in, 4, 0, out, 1, &read, &msg, false ) == ACN_ERR_ARG && says( msg, "handle" ) );
    EXPECT( lens( p, all, true, nullptr, 4, 0, out, 1, &read, &msg ) == ACN_ERR_ARG && says( msg, "null" ) && says( msg, "pos_xy" ) );
    EXPECT( lens( p, all, false, nullptr, 4, 0, out, 1, &read, &msg ) == ACN_OK );                        /* the main-pass form has no positions */
    EXPECT( lens( p, all, true, in, 4, 0, nullptr, 1, &read, &msg ) == ACN_ERR_ARG && says( msg, "null" ) && says( msg, "out" ) );
    EXPECT( lens( p, all, true, nullptr, 0, 0, nullptr, 1, &read, &msg ) == ACN_OK );
    { acn_lens_params q = p; q.samples = 4097; EXPECT( lens( q, all, true, in, 4, 0, out, 1, &read, &msg ) == ACN_ERR_ARG && says( msg, "samples" ) );
      EXPECT( lens( q, all, true, nullptr, 0, 0, nullptr, 1, &read, &msg ) == ACN_ERR_ARG );              /* (also with nothing to do) */
      q.samples = 4096; EXPECT( lens( q, all, true, in, 4, 0, out, 1, &read, &msg ) == ACN_OK ); }
    { acn_lens_params q = p; q.flags = 2; EXPECT( lens( q, all, true, in, 4, 0, out, 1, &read, &msg ) == ACN_ERR_ARG && says( msg, "flags" ) ); }
    for( double a : { -0.1, nan, inf, -inf } )
    {
        acn_lens_params q = p; q.aperture_radius = a;
        EXPECT( lens( q, all, true, in, 4, 0, out, 1, &read, &msg ) == ACN_ERR_ARG && says( msg, "aperture" ) );
    }
    for( double f : { 0.0, -1.0, nan, inf } )
    {
        acn_lens_params q = p; q.focus_distance = f;
        EXPECT( lens( q, all, true, in, 4, 0, out, 1, &read, &msg ) == ACN_ERR_ARG && says( msg, "focus" ) );
        q.aperture_radius = 0.0;                                                                         /* a closed aperture does not read it */
        EXPECT( lens( q, all, true, in, 4, 0, out, 1, &read, &msg ) == ACN_OK );
    }
    EXPECT( lens( p, all, true, in, 4, 2, out, 1, &read, &msg ) == ACN_ERR_ARG && says( msg, "mode" ) );
    EXPECT( lens( p, all, true, in, 4, 0xFFFFFFFFu, out, 1, &read, &msg ) == ACN_ERR_ARG && says( msg, "mode" ) );
    EXPECT( lens( p, all, true, in, 4, ACN_SURF_FOLLOW, out, 2, &read, &msg ) == ACN_ERR_ARG && says( msg, "sharded" ) );
    EXPECT( lens( p, all, true, ( const char* )in + 8, 4, 0, out, 1, &read, &msg ) == ACN_ERR_ARG && says( msg, "align" ) );
    EXPECT( lens( p, all, true, in, 4, 0, ( const char* )out + 8, 1, &read, &msg ) == ACN_ERR_ARG && says( msg, "align" ) );
    EXPECT( lens( p, all, false, ( const char* )in + 8, 4, 0, out, 1, &read, &msg ) == ACN_OK );          /* (positions that are not read) */
    EXPECT( lens( p, all, true, in, ( ( uint64_t )1 << 38 ) + 1, 0, out, 1, &read, &msg ) == ACN_ERR_ARG && says( msg, "2^38" ) );

    /* slices: floor( S / K ) positions, at least 1, at most n */
    EXPECT( acn_lenssurf_slice( ( size_t )1 << 21, 16, 1920 * 1080 ) == ( ( size_t )1 << 17 ) );
    EXPECT( acn_lenssurf_slice( 1024, 4, 600 ) == 256 && acn_lenssurf_slice( 1024, 5, 600 ) == 204 && acn_lenssurf_slice( 1024, 4, 100 ) == 100 );
    EXPECT( acn_lenssurf_slice( 1, 4096, 7 ) == 1 && acn_lenssurf_slice( 4095, 4096, 7 ) == 1 && acn_lenssurf_slice( 4096, 4096, 7 ) == 1 && acn_lenssurf_slice( 8192, 4096, 7 ) == 2 );
    EXPECT( acn_lenssurf_slice( 1024, 1, 0 ) == 0 );

    if( failures ) { printf( "%d checks failed\n", failures ); return 1; }
    printf( "ok\n" );
    return 0;
}
