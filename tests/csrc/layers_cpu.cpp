/* actinon_amd/csrc/acn_layers_host.h on its own: a program that tests/test_lens_layers_cpu.py builds with
 * -fsanitize=address,undefined and runs.  Every refusal of acn_lens_layers_reduce*, acn_render_lens_layers* and acn_denoise_layers*
 * that needs no handle, with each acn_lens_params in a heap block of exactly its struct_size, so a read past a short one is a
 * sanitizer report.  The program prints "ok" and returns 0, or names what failed. */
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <memory>

#include "acn_layers_host.h"

static int failures = 0;
#define EXPECT( cond ) do { if( !( cond ) ) { printf( "line %d: %s\n", __LINE__, #cond ); failures++; } } while( 0 )

static bool says( const std::string& msg, const char* word ) { return msg.find( word ) != std::string::npos; }

struct Shard { uint32_t mode, rank, world; };

/* the lens check with the first `bytes` bytes of p in a heap block of that size */
static int lens( const acn_lens_params& p, size_t bytes, bool need_pos, const void* pos, uint64_t n, uint32_t mode, const void* surf, const void* stats,
                 Shard sh, acn_lens_params* read, std::string* msg, bool have_handle = true )
{
    std::unique_ptr< unsigned char[] > block( new unsigned char[ bytes ] );
    memcpy( block.get(), &p, bytes );
    msg->clear();
    return acn_layers_lens_check( have_handle, need_pos, pos, n, ( const acn_lens_params* )block.get(), mode, surf, stats, sh.mode, sh.rank, sh.world, read, msg );
}

static int reduce( bool have_handle, const void* rec, const void* rad, uint64_t n, uint32_t K, const void* surf, const void* stats, uint32_t world, std::string* msg )
{
    msg->clear();
    return acn_layers_reduce_check( have_handle, rec, rad, n, K, surf, stats, world, msg );
}

int main()
{
    std::string msg;
    const double inf = std::numeric_limits< double >::infinity(), nan = std::nan( "" );
    alignas( 16 ) static double buf[ 128 ];
    const void* in = buf; const void* rad = buf + 32; const void* surf = buf + 64; const void* stats = buf + 96;
    const char* off8 = ( const char* )buf + 8;

    /* the reduce calls, in the order of the header */
    EXPECT( reduce( true, in, rad, 4, 16, surf, stats, 1, &msg ) == ACN_OK && msg.empty() );
    EXPECT( reduce( false, in, rad, 4, 16, surf, stats, 1, &msg ) == ACN_ERR_ARG && says( msg, "handle" ) );
    EXPECT( reduce( true, nullptr, rad, 4, 16, surf, stats, 1, &msg ) == ACN_ERR_ARG && says( msg, "null" ) && says( msg, "records" ) );
    EXPECT( reduce( true, in, nullptr, 4, 16, surf, stats, 1, &msg ) == ACN_ERR_ARG && says( msg, "null" ) && says( msg, "radiance" ) );
    EXPECT( reduce( true, in, rad, 4, 16, nullptr, stats, 1, &msg ) == ACN_ERR_ARG && says( msg, "null" ) && says( msg, "out_surface" ) );
    EXPECT( reduce( true, in, rad, 4, 16, surf, nullptr, 1, &msg ) == ACN_ERR_ARG && says( msg, "null" ) && says( msg, "out_stats" ) );
    EXPECT( reduce( true, nullptr, nullptr, 0, 16, nullptr, nullptr, 0, &msg ) == ACN_OK );
    EXPECT( reduce( true, in, rad, 4, 0, surf, stats, 1, &msg ) == ACN_ERR_ARG && says( msg, "K 0" ) );
    EXPECT( reduce( true, nullptr, nullptr, 0, 0, nullptr, nullptr, 1, &msg ) == ACN_ERR_ARG && says( msg, "K 0" ) );   /* (also with nothing to do) */
    EXPECT( reduce( true, in, rad, 4, 4097, surf, stats, 1, &msg ) == ACN_ERR_ARG && says( msg, "4097" ) );
    EXPECT( reduce( true, in, rad, 4, 0xFFFFFFFFu, surf, stats, 1, &msg ) == ACN_ERR_ARG );
    EXPECT( reduce( true, in, rad, 4, 1, surf, stats, 1, &msg ) == ACN_OK && reduce( true, in, rad, 4, 4096, surf, stats, 1, &msg ) == ACN_OK );
    EXPECT( reduce( true, in, rad, 4, 16, surf, stats, 2, &msg ) == ACN_ERR_ARG && says( msg, "sharded" ) );
    EXPECT( reduce( true, off8, rad, 4, 16, surf, stats, 1, &msg ) == ACN_ERR_ARG && says( msg, "align" ) );
    EXPECT( reduce( true, in, rad, 4, 16, ( const char* )surf + 8, stats, 1, &msg ) == ACN_ERR_ARG && says( msg, "align" ) );
    EXPECT( reduce( true, in, rad, 4, 16, surf, ( const char* )stats + 8, 1, &msg ) == ACN_ERR_ARG && says( msg, "align" ) );
    EXPECT( reduce( true, in, ( const char* )rad + 8, 4, 16, surf, stats, 1, &msg ) == ACN_OK );                       /* radiances are doubles */
    EXPECT( reduce( true, in, ( const char* )rad + 4, 4, 16, surf, stats, 1, &msg ) == ACN_ERR_ARG && says( msg, "align" ) );
    EXPECT( reduce( true, in, rad, ( ( uint64_t )1 << 38 ) + 1, 16, surf, stats, 1, &msg ) == ACN_ERR_ARG && says( msg, "2^38" ) );
    EXPECT( reduce( true, in, rad, ( uint64_t )1 << 38, 16, surf, stats, 1, &msg ) == ACN_OK );

    /* the lens calls: every layout a caller may have been compiled with */
    const Shard none = { ACN_SHARD_NONE, 0, 0 };
    acn_lens_params p = ACN_LENS_PARAMS_INIT, read;
    p.samples = 8; p.flags = ACN_LENS_JITTER; p.seed = 5; p.aperture_radius = 0.25; p.focus_distance = 12.0;
    for( uint32_t size = 0; size <= sizeof( p ) + 8; size++ )
    {
        acn_lens_params q = p;
        q.struct_size = size;
        const size_t have = size < sizeof( q ) ? ( size < 4 ? 4 : size ) : sizeof( q );
        const int st = lens( q, have, true, in, 4, ACN_SURF_FOLLOW, surf, stats, none, &read, &msg );
        if( size < 4 ) { EXPECT( st == ACN_ERR_ARG && says( msg, "struct_size" ) ); continue; }
        if( size % 4 || ( size > 16 && size % 8 ) ) continue;   /* (a size inside a member: part of its bytes) */
        if( size >= 24 && size < 32 ) { EXPECT( st == ACN_ERR_ARG && says( msg, "focus" ) ); continue; }   /* an aperture without its focus */
        EXPECT( st == ACN_OK );
        EXPECT( read.samples == ( size >= 8 ? 8u : 0u ) && read.flags == ( size >= 12 ? ACN_LENS_JITTER : 0u ) && read.seed == ( size >= 16 ? 5u : 0u ) );
        EXPECT( read.aperture_radius == ( size >= 24 ? 0.25 : 0.0 ) && read.focus_distance == ( size >= 32 ? 12.0 : 0.0 ) );
    }
    msg.clear();
    EXPECT( acn_layers_lens_check( true, true, in, 4, nullptr, ACN_SURF_FIRST_HIT, surf, stats, 0, 0, 0, &read, &msg ) == ACN_OK && read.samples == 0 && read.aperture_radius == 0.0 );
    /* the refusals, in the order of the header */
    const size_t all = sizeof( p );
    EXPECT( lens( p, all, true, in, 4, 0, surf, stats, none, &read, &msg, false ) == ACN_ERR_ARG && says( msg, "handle" ) );
    EXPECT( lens( p, all, true, nullptr, 4, 0, surf, stats, none, &read, &msg ) == ACN_ERR_ARG && says( msg, "null" ) && says( msg, "pos_xy" ) );
    EXPECT( lens( p, all, false, nullptr, 4, 0, surf, stats, none, &read, &msg ) == ACN_OK );                          /* the main-pass form has no positions */
    EXPECT( lens( p, all, true, in, 4, 0, nullptr, stats, none, &read, &msg ) == ACN_ERR_ARG && says( msg, "null" ) && says( msg, "out_surface" ) );
    EXPECT( lens( p, all, true, in, 4, 0, surf, nullptr, none, &read, &msg ) == ACN_ERR_ARG && says( msg, "null" ) && says( msg, "out_stats" ) );
    EXPECT( lens( p, all, true, nullptr, 0, 0, nullptr, nullptr, none, &read, &msg ) == ACN_OK );
    { acn_lens_params q = p; q.samples = 4097; EXPECT( lens( q, all, true, in, 4, 0, surf, stats, none, &read, &msg ) == ACN_ERR_ARG && says( msg, "samples" ) );
      EXPECT( lens( q, all, true, nullptr, 0, 0, nullptr, nullptr, none, &read, &msg ) == ACN_ERR_ARG );              /* (also with nothing to do) */
      q.samples = 4096; EXPECT( lens( q, all, true, in, 4, 0, surf, stats, none, &read, &msg ) == ACN_OK ); }
    { acn_lens_params q = p; q.flags = 2; EXPECT( lens( q, all, true, in, 4, 0, surf, stats, none, &read, &msg ) == ACN_ERR_ARG && says( msg, "flags" ) ); }
    for( double a : { -0.1, nan, inf, -inf } )
    {
        acn_lens_params q = p; q.aperture_radius = a;
        EXPECT( lens( q, all, true, in, 4, 0, surf, stats, none, &read, &msg ) == ACN_ERR_ARG && says( msg, "aperture" ) );
    }
    for( double f : { 0.0, -1.0, nan, inf } )
    {
        acn_lens_params q = p; q.focus_distance = f;
        EXPECT( lens( q, all, true, in, 4, 0, surf, stats, none, &read, &msg ) == ACN_ERR_ARG && says( msg, "focus" ) );
        q.aperture_radius = 0.0;                                                                                      /* a closed aperture does not read it */
        EXPECT( lens( q, all, true, in, 4, 0, surf, stats, none, &read, &msg ) == ACN_OK );
    }
    EXPECT( lens( p, all, true, in, 4, 2, surf, stats, none, &read, &msg ) == ACN_ERR_ARG && says( msg, "mode" ) );
    EXPECT( lens( p, all, true, in, 4, 0xFFFFFFFFu, surf, stats, none, &read, &msg ) == ACN_ERR_ARG && says( msg, "mode" ) );
    EXPECT( lens( p, all, true, in, 4, 1, surf, stats, Shard{ 2, 0, 1 }, &read, &msg ) == ACN_ERR_ARG && says( msg, "shard_mode" ) );
    EXPECT( lens( p, all, true, in, 4, 1, surf, stats, Shard{ ACN_SHARD_SAMPLES, 0, 2 }, &read, &msg ) == ACN_ERR_ARG && says( msg, "ACN_SHARD_SAMPLES" ) );
    EXPECT( lens( p, all, true, in, 4, 1, surf, stats, Shard{ ACN_SHARD_SAMPLES, 2, 2 }, &read, &msg ) == ACN_ERR_ARG && says( msg, "shard_rank" ) );
    EXPECT( lens( p, all, true, in, 4, 1, surf, stats, Shard{ ACN_SHARD_SAMPLES, 0, 1 }, &read, &msg ) == ACN_OK );     /* a world of one is not sharded */
    EXPECT( lens( p, all, true, in, 4, 1, surf, stats, Shard{ ACN_SHARD_SAMPLES, 0, 0 }, &read, &msg ) == ACN_OK );
    EXPECT( lens( p, all, true, off8, 4, 0, surf, stats, none, &read, &msg ) == ACN_ERR_ARG && says( msg, "align" ) );
    EXPECT( lens( p, all, true, in, 4, 0, ( const char* )surf + 8, stats, none, &read, &msg ) == ACN_ERR_ARG && says( msg, "align" ) );
    EXPECT( lens( p, all, true, in, 4, 0, surf, ( const char* )stats + 8, none, &read, &msg ) == ACN_ERR_ARG && says( msg, "align" ) );
    EXPECT( lens( p, all, false, off8, 4, 0, surf, stats, none, &read, &msg ) == ACN_OK );                             /* (positions that are not read) */
    EXPECT( lens( p, all, true, in, ( ( uint64_t )1 << 38 ) + 1, 0, surf, stats, none, &read, &msg ) == ACN_ERR_ARG && says( msg, "2^38" ) );

    /* the planes of the layered filter */
    msg.clear();
    EXPECT( acn_layers_denoise_check( stats, surf, &msg ) == ACN_OK && msg.empty() );
    EXPECT( acn_layers_denoise_check( ( const char* )stats + 8, surf, &msg ) == ACN_ERR_ARG && says( msg, "statistics" ) && says( msg, "align" ) );
    EXPECT( acn_layers_denoise_check( stats, ( const char* )surf + 8, &msg ) == ACN_ERR_ARG && says( msg, "surface" ) && says( msg, "align" ) );

    if( failures ) { printf( "%d checks failed\n", failures ); return 1; }
    printf( "ok\n" );
    return 0;
}
