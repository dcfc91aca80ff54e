/* test program: the host-side checks of the lens statistics entry points (actinon_amd/csrc/acn_stats_host.h) on their own, built with
 * -fsanitize=address,undefined by tests/test_lens_stats_cpu.py.  Every input lives in a heap block of exactly its size, so a read
 * past a short acn_lens_params or past the last index is a sanitizer report.  Prints "ok" and returns 0, or names what failed. */
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <memory>

#include "acn_stats_host.h"

static int failures = 0;
#define EXPECT( cond ) do { if( !( cond ) ) { printf( "line %d: %s\n", __LINE__, #cond ); failures++; } } while( 0 )

/* the first `bytes` bytes of p in a heap block of that size */
static std::unique_ptr< unsigned char[] > exact( const acn_lens_params& p, size_t bytes )
{
    std::unique_ptr< unsigned char[] > b( new unsigned char[ bytes ] );
    memcpy( b.get(), &p, bytes );
    return b;
}

static int read_params( const acn_lens_params& p, size_t bytes, acn_lens_params* out, std::string* msg )
{
    auto block = exact( p, bytes );
    return acn_lens_params_read( ( const acn_lens_params* )block.get(), out, msg );
}

static int check_index( const std::vector< int64_t >& idx, size_t n_acc, std::string* msg )
{
    std::unique_ptr< int64_t[] > block( new int64_t[ idx.size() ? idx.size() : 1 ] );
    for( size_t i = 0; i < idx.size(); i++ ) block[ i ] = idx[ i ];
    return acn_stats_index_check( block.get(), idx.size(), n_acc, msg );
}

int main()
{
    std::string msg;
    acn_lens_params out;
    const double inf = std::numeric_limits< double >::infinity(), nan = std::nan( "" );

    /* params: null, whole, and every shorter layout a caller may have been compiled with */
    EXPECT( acn_lens_params_read( nullptr, &out, &msg ) == ACN_OK && out.samples == 0 && out.flags == 0 && out.aperture_radius == 0.0 );
    acn_lens_params p = ACN_LENS_PARAMS_INIT;
    p.samples = 7; p.flags = ACN_LENS_JITTER; p.seed = 5; p.aperture_radius = 0.25; p.focus_distance = 3.0;
    EXPECT( read_params( p, sizeof( p ), &out, &msg ) == ACN_OK && out.samples == 7 && out.seed == 5 && out.focus_distance == 3.0 );
    for( uint32_t size = 0; size <= sizeof( p ) + 8; size++ )
    {
        acn_lens_params q = p;
        q.struct_size = size;
        const size_t have = size < sizeof( q ) ? ( size < 4 ? 4 : size ) : sizeof( q );   /* the block the caller really owns */
        msg.clear();
        const int st = read_params( q, have, &out, &msg );
        if( size < 4 ) { EXPECT( st == ACN_ERR_ARG && msg.find( "struct_size" ) != std::string::npos ); continue; }
        if( size % 4 ) { EXPECT( st == ACN_OK || st == ACN_ERR_ARG ); continue; }   /* (a size inside a member: part of its bytes) */
        /* (a caller that knows the aperture but not the focus distance opens the lens without one) */
        if( size >= 24 && size < 32 ) { EXPECT( st == ACN_ERR_ARG && msg.find( "focus" ) != std::string::npos ); continue; }
        if( size > 16 && size < 24 ) continue;                                        /* (half an aperture) */
        EXPECT( st == ACN_OK );
        EXPECT( out.samples == ( size >= 8 ? 7u : 0u ) && out.flags == ( size >= 12 ? ACN_LENS_JITTER : 0u ) && out.seed == ( size >= 16 ? 5u : 0u ) );
        EXPECT( out.aperture_radius == ( size >= 24 ? 0.25 : 0.0 ) && out.focus_distance == ( size >= 32 ? 3.0 : 0.0 ) );
    }
    struct { uint32_t samples, flags; double aperture, focus; const char* word; } bad[] = {
        { 4097, 0, 0.0, 0.0, "samples" }, { 4, 2, 0.0, 0.0, "flags" }, { 4, 0x80000000u, 0.0, 0.0, "flags" },
        { 4, 0, -0.1, 1.0, "aperture" }, { 4, 0, nan, 1.0, "aperture" }, { 4, 0, inf, 1.0, "aperture" },
        { 4, 0, 0.1, 0.0, "focus" }, { 4, 0, 0.1, -3.0, "focus" }, { 4, 0, 0.1, inf, "focus" }, { 4, 0, 0.1, nan, "focus" } };
    for( const auto& b : bad )
    {
        acn_lens_params q = ACN_LENS_PARAMS_INIT;
        q.samples = b.samples; q.flags = b.flags; q.aperture_radius = b.aperture; q.focus_distance = b.focus;
        msg.clear();
        EXPECT( read_params( q, sizeof( q ), &out, &msg ) == ACN_ERR_ARG && msg.find( b.word ) != std::string::npos );
    }
    { acn_lens_params q = ACN_LENS_PARAMS_INIT; q.samples = 4096; q.focus_distance = nan; EXPECT( read_params( q, sizeof( q ), &out, &msg ) == ACN_OK ); }

    /* indices */
    const int64_t lo = std::numeric_limits< int64_t >::min(), hi = std::numeric_limits< int64_t >::max();
    EXPECT( acn_stats_index_check( nullptr, 0, 0, &msg ) == ACN_OK );
    EXPECT( acn_stats_index_check( nullptr, 5, 5, &msg ) == ACN_OK );
    EXPECT( acn_stats_index_check( nullptr, 6, 5, &msg ) == ACN_ERR_ARG && msg.find( "n_part" ) != std::string::npos );
    EXPECT( check_index( {}, 0, &msg ) == ACN_OK );
    EXPECT( check_index( { 4, 0, 2, 1, 3 }, 5, &msg ) == ACN_OK );
    EXPECT( check_index( { 0 }, 1, &msg ) == ACN_OK );
    EXPECT( check_index( { 0 }, 0, &msg ) == ACN_ERR_ARG && msg.find( "out of range" ) != std::string::npos );
    for( int64_t v : { ( int64_t )-1, ( int64_t )5, lo, hi, ( int64_t )1 << 32 } )
    {
        msg.clear();
        EXPECT( check_index( { 0, 1, v, 2 }, 5, &msg ) == ACN_ERR_ARG && msg.find( "out of range" ) != std::string::npos && msg.find( "index[ 2 ]" ) != std::string::npos );
    }
    msg.clear();
    EXPECT( check_index( { 3, 1, 4, 1 }, 5, &msg ) == ACN_ERR_ARG && msg.find( "duplicate" ) != std::string::npos && msg.find( "index[ 3 ]" ) != std::string::npos );
    EXPECT( check_index( { 4, 4 }, 5, &msg ) == ACN_ERR_ARG );
    {   /* a long one: every index of a large accumulator, backwards, then one of them again */
        std::vector< int64_t > all( 100000 );
        for( size_t i = 0; i < all.size(); i++ ) all[ i ] = ( int64_t )( all.size() - 1 - i );
        EXPECT( check_index( all, all.size(), &msg ) == ACN_OK );
        all.push_back( 77 );
        EXPECT( check_index( all, all.size(), &msg ) == ACN_ERR_ARG && msg.find( "duplicate" ) != std::string::npos );
    }

    /* buffers */
    alignas( 64 ) static double block[ 16 ];
    EXPECT( acn_stats_buffer_check( block, 2, "d_stats", &msg ) == ACN_OK );
    EXPECT( acn_stats_buffer_check( block + 2, 1, "d_stats", &msg ) == ACN_OK );
    msg.clear();
    EXPECT( acn_stats_buffer_check( block + 1, 1, "d_stats", &msg ) == ACN_ERR_ARG && msg.find( "align" ) != std::string::npos );
    EXPECT( acn_stats_buffer_check( nullptr, 1, "d_stats", &msg ) == ACN_ERR_ARG && msg.find( "null" ) != std::string::npos );
    EXPECT( acn_stats_buffer_check( nullptr, 0, "d_stats", &msg ) == ACN_OK );
    EXPECT( acn_stats_buffer_check( block, ( ( size_t )1 << 38 ) + 1, "d_stats", &msg ) == ACN_ERR_ARG );

    if( failures ) { printf( "%d checks failed\n", failures ); return 1; }
    printf( "ok\n" );
    return 0;
}
