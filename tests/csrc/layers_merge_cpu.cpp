/* the checks of acn_lens_layers_merge* and acn_lens_layers_resolve_dev in actinon_amd/csrc/acn_layers_host.h on their own: a program
 * that tests/test_lens_layers_merge_cpu.py builds with -fsanitize=address,undefined and runs.  Every refusal that needs no handle, with
 * each index list in a heap block of exactly its size, so a read past it is a sanitizer report.  The program prints "ok" and
 * returns 0, or names what failed. */
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "acn_layers_host.h"

static int failures = 0;
#define EXPECT( cond ) do { if( !( cond ) ) { printf( "line %d: %s\n", __LINE__, #cond ); failures++; } } while( 0 )

static bool says( const std::string& msg, const char* word ) { return msg.find( word ) != std::string::npos; }

struct Planes { const void* as; const void* at; const void* ps; const void* pt; };

static int merge( const Planes& p, uint64_t n_acc, uint64_t n_part, const int64_t* index, bool host, std::string* msg, bool have_handle = true, uint32_t world = 1 )
{
    msg->clear();
    return acn_layers_merge_check( have_handle, p.as, p.at, n_acc, p.ps, p.pt, n_part, index, host, world, msg );
}

/* the host form's check with the list in a heap block of exactly n_part entries */
static int merge_list( const Planes& p, uint64_t n_acc, const std::vector< int64_t >& list, std::string* msg )
{
    std::unique_ptr< int64_t[] > block( new int64_t[ list.size() ? list.size() : 1 ] );
    for( size_t k = 0; k < list.size(); k++ ) block[ k ] = list[ k ];
    return merge( p, n_acc, list.size(), block.get(), true, msg );
}

static int resolve( const void* stats, uint64_t n, const void* rgb, const void* noise, const void* pooled, std::string* msg, bool have_handle = true, uint32_t world = 1 )
{
    msg->clear();
    return acn_layers_resolve_check( have_handle, stats, n, rgb, noise, pooled, world, msg );
}

int main()
{
    std::string msg;
    alignas( 16 ) static double buf[ 256 ];
    const Planes good = { buf, buf + 64, buf + 128, buf + 192 };
    const char* off8 = ( const char* )buf + 8;
    alignas( 16 ) static int64_t dev_index[ 4 ] = { 0, 0, -7, 1000 };   /* (a device list is never read here: duplicates and ranges pass) */

    /* the merge, in the order of the header */
    EXPECT( merge( good, 8, 4, nullptr, false, &msg ) == ACN_OK && msg.empty() );
    EXPECT( merge( good, 8, 4, nullptr, false, &msg, false ) == ACN_ERR_ARG && says( msg, "handle" ) );
    { Planes p = good; p.as = nullptr; EXPECT( merge( p, 8, 4, nullptr, false, &msg ) == ACN_ERR_ARG && says( msg, "null" ) && says( msg, "acc_surface" ) ); }
    { Planes p = good; p.at = nullptr; EXPECT( merge( p, 8, 4, nullptr, false, &msg ) == ACN_ERR_ARG && says( msg, "null" ) && says( msg, "acc_stats" ) ); }
    { Planes p = good; p.ps = nullptr; EXPECT( merge( p, 8, 4, nullptr, false, &msg ) == ACN_ERR_ARG && says( msg, "null" ) && says( msg, "part_surface" ) ); }
    { Planes p = good; p.pt = nullptr; EXPECT( merge( p, 8, 4, nullptr, false, &msg ) == ACN_ERR_ARG && says( msg, "null" ) && says( msg, "part_stats" ) ); }
    { Planes p = { buf, buf + 64, nullptr, nullptr }; EXPECT( merge( p, 8, 0, nullptr, false, &msg ) == ACN_OK ); }                  /* nothing to merge */
    { Planes p = { nullptr, nullptr, nullptr, nullptr }; EXPECT( merge( p, 0, 0, nullptr, false, &msg ) == ACN_OK ); }
    EXPECT( merge( good, 8, 4, nullptr, false, &msg, true, 2 ) == ACN_ERR_ARG && says( msg, "sharded" ) );
    for( int which = 0; which < 4; which++ )
    {
        Planes p = good;
        ( which == 0 ? p.as : which == 1 ? p.at : which == 2 ? p.ps : p.pt ) = off8 + which * 512;
        EXPECT( merge( p, 8, 4, nullptr, false, &msg ) == ACN_ERR_ARG && says( msg, "align" ) );
    }
    EXPECT( merge( good, 8, 4, ( const int64_t* )( ( const char* )dev_index + 4 ), false, &msg ) == ACN_ERR_ARG && says( msg, "int64_t" ) );
    EXPECT( merge( good, 8, 4, dev_index, false, &msg ) == ACN_OK );
    EXPECT( merge( good, 2, 4, dev_index, false, &msg ) == ACN_OK );                                                                  /* with an index the part may be longer */
    EXPECT( merge( good, ( ( uint64_t )1 << 38 ) + 1, 4, dev_index, false, &msg ) == ACN_ERR_ARG && says( msg, "2^38" ) );
    EXPECT( merge( good, 8, ( ( uint64_t )1 << 38 ) + 1, dev_index, false, &msg ) == ACN_ERR_ARG && says( msg, "2^38" ) );
    /* a null index: the part must fit, in either form */
    EXPECT( merge( good, 4, 4, nullptr, false, &msg ) == ACN_OK && merge( good, 4, 4, nullptr, true, &msg ) == ACN_OK );
    EXPECT( merge( good, 3, 4, nullptr, false, &msg ) == ACN_ERR_ARG && says( msg, "n_part <= n_acc" ) );
    EXPECT( merge( good, 3, 4, nullptr, true, &msg ) == ACN_ERR_ARG && says( msg, "n_part <= n_acc" ) );
    /* the host form reads its list: in range, none twice */
    EXPECT( merge_list( good, 8, { 7, 0, 3 }, &msg ) == ACN_OK && msg.empty() );
    EXPECT( merge_list( good, 2, { 1, 0 }, &msg ) == ACN_OK );
    EXPECT( merge_list( good, 8, { 7, 8, 3 }, &msg ) == ACN_ERR_ARG && says( msg, "index[ 1 ] = 8" ) && says( msg, "out of range" ) );
    EXPECT( merge_list( good, 8, { -1 }, &msg ) == ACN_ERR_ARG && says( msg, "out of range" ) );
    EXPECT( merge_list( good, 8, { 1, 2, 1 }, &msg ) == ACN_ERR_ARG && says( msg, "index[ 2 ] = 1" ) && says( msg, "duplicate" ) );
    EXPECT( merge_list( good, 8, { INT64_MIN, INT64_MAX }, &msg ) == ACN_ERR_ARG && says( msg, "out of range" ) );
    EXPECT( merge_list( good, 8, {}, &msg ) == ACN_OK );

    /* the resolve */
    const void* stats = buf; const void* rgb = buf + 64; const void* noise = buf + 128; const void* pooled = buf + 192;
    EXPECT( resolve( stats, 4, rgb, noise, pooled, &msg ) == ACN_OK && msg.empty() );
    EXPECT( resolve( stats, 4, nullptr, nullptr, nullptr, &msg ) == ACN_OK );                                                         /* every output is nullable */
    EXPECT( resolve( stats, 4, rgb, noise, pooled, &msg, false ) == ACN_ERR_ARG && says( msg, "handle" ) );
    EXPECT( resolve( nullptr, 4, rgb, noise, pooled, &msg ) == ACN_ERR_ARG && says( msg, "null" ) && says( msg, "stats" ) );
    EXPECT( resolve( nullptr, 0, nullptr, nullptr, nullptr, &msg ) == ACN_OK );
    EXPECT( resolve( stats, 4, rgb, noise, pooled, &msg, true, 2 ) == ACN_ERR_ARG && says( msg, "sharded" ) );
    EXPECT( resolve( off8, 4, rgb, noise, pooled, &msg ) == ACN_ERR_ARG && says( msg, "align" ) );
    EXPECT( resolve( stats, 4, rgb, noise, ( const char* )pooled + 8, &msg ) == ACN_ERR_ARG && says( msg, "align" ) );
    EXPECT( resolve( stats, 4, ( const char* )rgb + 8, ( const char* )noise + 8, pooled, &msg ) == ACN_OK );                          /* arrays of doubles */
    EXPECT( resolve( stats, 4, ( const char* )rgb + 4, noise, pooled, &msg ) == ACN_ERR_ARG && says( msg, "align" ) );
    EXPECT( resolve( stats, 4, rgb, ( const char* )noise + 4, pooled, &msg ) == ACN_ERR_ARG && says( msg, "align" ) );
    EXPECT( resolve( stats, ( ( uint64_t )1 << 38 ) + 1, rgb, noise, pooled, &msg ) == ACN_ERR_ARG && says( msg, "2^38" ) );

    if( failures ) { printf( "%d checks failed\n", failures ); return 1; }
    printf( "ok\n" );
    return 0;
}
