/* actinon_amd/csrc/acn_select_host.h on its own, twice.  As a shared library it is the extern "C" shim through which
 * tests/test_select_cpu.py compares the host arithmetic with tests/select_model.py.  With -DSELECT_CPU_MAIN it is a program that
 * the same test builds with -fsanitize=address,undefined and runs: every refusal of the two calls, with each input in a heap block
 * of exactly its size, so a read past a short acn_select_params or past word 256 of a histogram is a sanitizer report.  The program
 * prints "ok" and returns 0, or names what failed. */
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <memory>
#include <vector>

#include "acn_select_host.h"

static void put( const std::string& msg, char* out, size_t room )
{
    if( !out || !room ) return;
    const size_t len = msg.size() < room - 1 ? msg.size() : room - 1;
    memcpy( out, msg.data(), len );
    out[ len ] = 0;
}

extern "C"
{
double sel_edge( uint32_t bin ) { return acn_select_hist_edge( bin ); }
void sel_bins( const uint64_t* bits, size_t n, uint32_t* out ) { for( size_t i = 0; i < n; i++ ) out[ i ] = acn_select_key_bin( bits[ i ] ); }
double sel_threshold( const uint64_t* hist, uint64_t budget ) { return acn_select_hist_threshold( hist, budget ); }
uint64_t sel_tile( void ) { return ACN_SELECT_TILE; }
uint64_t sel_tiles( uint64_t n ) { return acn_select_tiles( n ); }
/* *out is written only when the call is accepted; msg only when it is refused */
int sel_check_select( int have_handle, const void* key, uint64_t n, const acn_select_params* prm, const void* src_pos_xy, const void* out_index,
                      const void* out_pos_xy, uint32_t shard_world, acn_select_params* out, char* msg, size_t msg_room )
{
    std::string m;
    acn_select_params p;
    const int st = acn_select_args_check( have_handle != 0, key, n, prm, src_pos_xy, out_index, out_pos_xy, shard_world, &p, &m );
    if( st == ACN_OK ) *out = p; else put( m, msg, msg_room );
    return st;
}
int sel_check_hist( int have_handle, const void* key, uint64_t n, const void* out_hist, uint32_t shard_world, char* msg, size_t msg_room )
{
    std::string m;
    const int st = acn_key_hist_args_check( have_handle != 0, key, n, out_hist, shard_world, &m );
    if( st != ACN_OK ) put( m, msg, msg_room );
    return st;
}
}

#ifdef SELECT_CPU_MAIN
static int failures = 0;
#define EXPECT( cond ) do { if( !( cond ) ) { printf( "line %d: %s\n", __LINE__, #cond ); failures++; } } while( 0 )

/* the check with the first `bytes` bytes of p in a heap block of that size */
static int check( const acn_select_params& p, size_t bytes, const void* key, uint64_t n, const void* src, const void* idx, const void* pos,
                  uint32_t world, acn_select_params* out, std::string* msg, bool have_handle = true )
{
    std::unique_ptr< unsigned char[] > block( new unsigned char[ bytes ] );
    memcpy( block.get(), &p, bytes );
    msg->clear();
    return acn_select_args_check( have_handle, key, n, ( const acn_select_params* )block.get(), src, idx, pos, world, out, msg );
}

static bool says( const std::string& msg, const char* word ) { return msg.find( word ) != std::string::npos; }

int main()
{
    std::string msg;
    acn_select_params out;
    const double inf = std::numeric_limits< double >::infinity(), nan = std::nan( "" );
    alignas( 16 ) static double buf[ 8 ];
    const void* key = buf; const void* pos = buf + 2; const void* idx = buf + 4;

    /* every layout a caller may have been compiled with */
    acn_select_params p = ACN_SELECT_PARAMS_INIT;
    p.threshold = 0.25; p.capacity = 7; p.raster_width = 5; p.raster_first = 3;
    for( uint32_t size = 0; size <= sizeof( p ) + 8; size++ )
    {
        acn_select_params q = p;
        q.struct_size = size;
        const size_t have = size < sizeof( q ) ? ( size < 4 ? 4 : size ) : sizeof( q );
        const int st = check( q, have, key, 4, nullptr, idx, pos, 1, &out, &msg );
        if( size < 16 ) { EXPECT( st == ACN_ERR_ARG && says( msg, "struct_size" ) ); continue; }
        if( size % 8 ) continue;   /* (a size inside a member: part of its bytes) */
        EXPECT( st == ACN_OK && out.threshold == 0.25 );
        EXPECT( out.capacity == ( size >= 24 ? 7u : 0u ) && out.raster_width == ( size >= 32 ? 5u : 0u ) && out.raster_first == ( size >= 40 ? 3u : 0u ) );
    }
    /* the refusals, in the order of the header */
    EXPECT( check( p, sizeof( p ), key, 4, nullptr, idx, pos, 1, &out, &msg, false ) == ACN_ERR_ARG && says( msg, "handle" ) );
    EXPECT( check( p, sizeof( p ), nullptr, 4, nullptr, idx, pos, 1, &out, &msg ) == ACN_ERR_ARG && says( msg, "key" ) );
    EXPECT( check( p, sizeof( p ), nullptr, 0, nullptr, idx, pos, 1, &out, &msg ) == ACN_OK );
    EXPECT( check( p, sizeof( p ), key, ( ( uint64_t )1 << 31 ) + 1, nullptr, idx, pos, 1, &out, &msg ) == ACN_ERR_ARG && says( msg, "2^31" ) );
    EXPECT( check( p, sizeof( p ), key, ( uint64_t )1 << 31, nullptr, idx, pos, 1, &out, &msg ) == ACN_OK );
    msg.clear();
    EXPECT( acn_select_args_check( true, key, 4, nullptr, nullptr, idx, pos, 1, &out, &msg ) == ACN_ERR_ARG && says( msg, "acn_select_params" ) );
    { acn_select_params q = p; q.flags = 1; EXPECT( check( q, sizeof( q ), key, 4, nullptr, idx, pos, 1, &out, &msg ) == ACN_ERR_ARG && says( msg, "flags" ) ); }
    { acn_select_params q = p; q.flags = 0x80000000u; EXPECT( check( q, sizeof( q ), key, 4, nullptr, idx, pos, 1, &out, &msg ) == ACN_ERR_ARG && says( msg, "flags" ) ); }
    { acn_select_params q = p; q.threshold = nan; EXPECT( check( q, sizeof( q ), key, 4, nullptr, idx, pos, 1, &out, &msg ) == ACN_ERR_ARG && says( msg, "NaN" ) ); }
    { acn_select_params q = p; q.threshold = -nan; EXPECT( check( q, sizeof( q ), key, 4, nullptr, idx, pos, 1, &out, &msg ) == ACN_ERR_ARG && says( msg, "NaN" ) ); }
    for( double t : { inf, -inf, 0.0, -0.0, 5e-324 } )
    {
        acn_select_params q = p; q.threshold = t;
        EXPECT( check( q, sizeof( q ), key, 4, nullptr, idx, pos, 1, &out, &msg ) == ACN_OK && memcmp( &out.threshold, &t, 8 ) == 0 );
    }
    EXPECT( check( p, sizeof( p ), key, 4, nullptr, nullptr, nullptr, 1, &out, &msg ) == ACN_ERR_ARG && says( msg, "capacity" ) );
    EXPECT( check( p, sizeof( p ), key, 4, nullptr, idx, nullptr, 1, &out, &msg ) == ACN_OK );
    EXPECT( check( p, sizeof( p ), key, 4, nullptr, nullptr, pos, 1, &out, &msg ) == ACN_OK );
    { acn_select_params q = p; q.capacity = 0; EXPECT( check( q, sizeof( q ), key, 4, nullptr, nullptr, nullptr, 0, &out, &msg ) == ACN_OK ); }   /* a pure count */
    EXPECT( check( p, sizeof( p ), key, 4, nullptr, idx, pos, 2, &out, &msg ) == ACN_ERR_ARG && says( msg, "sharded" ) );
    EXPECT( check( p, sizeof( p ), ( const char* )key + 4, 4, nullptr, idx, pos, 1, &out, &msg ) == ACN_ERR_ARG && says( msg, "align" ) );
    EXPECT( check( p, sizeof( p ), key, 4, nullptr, ( const char* )idx + 1, pos, 1, &out, &msg ) == ACN_ERR_ARG && says( msg, "align" ) );
    { acn_select_params q = p; q.raster_first = ( ( uint64_t )1 << 52 ) - 3; EXPECT( check( q, sizeof( q ), key, 4, nullptr, idx, pos, 1, &out, &msg ) == ACN_ERR_ARG && says( msg, "2^52" ) );
      EXPECT( check( q, sizeof( q ), key, 3, nullptr, idx, pos, 1, &out, &msg ) == ACN_OK );
      EXPECT( check( q, sizeof( q ), key, 4, pos, idx, pos, 1, &out, &msg ) == ACN_OK );          /* (gathered positions: the raster is not used) */
      q.raster_first = ~( uint64_t )0; EXPECT( check( q, sizeof( q ), key, 4, nullptr, idx, pos, 1, &out, &msg ) == ACN_ERR_ARG ); }

    /* the histogram call */
    msg.clear(); EXPECT( acn_key_hist_args_check( false, key, 4, buf, 1, &msg ) == ACN_ERR_ARG && says( msg, "handle" ) );
    msg.clear(); EXPECT( acn_key_hist_args_check( true, nullptr, 4, buf, 1, &msg ) == ACN_ERR_ARG && says( msg, "key" ) );
    msg.clear(); EXPECT( acn_key_hist_args_check( true, key, 4, nullptr, 1, &msg ) == ACN_ERR_ARG && says( msg, "out_hist" ) );
    msg.clear(); EXPECT( acn_key_hist_args_check( true, key, ( ( uint64_t )1 << 31 ) + 1, buf, 1, &msg ) == ACN_ERR_ARG && says( msg, "2^31" ) );
    msg.clear(); EXPECT( acn_key_hist_args_check( true, key, 4, buf, 3, &msg ) == ACN_ERR_ARG && says( msg, "sharded" ) );
    msg.clear(); EXPECT( acn_key_hist_args_check( true, key, 4, ( const char* )buf + 4, 1, &msg ) == ACN_ERR_ARG && says( msg, "align" ) );
    EXPECT( acn_key_hist_args_check( true, nullptr, 0, buf, 0, &msg ) == ACN_OK );

    /* edges, bins and thresholds: the words at the ends, in blocks of exactly 257 words */
    EXPECT( acn_select_hist_edge( 0 ) == -inf && std::isnan( acn_select_hist_edge( 256 ) ) && std::isnan( acn_select_hist_edge( 0xFFFFFFFFu ) ) );
    EXPECT( acn_select_hist_edge( 1 ) == std::ldexp( 1.0, -40 ) && acn_select_hist_edge( 5 ) == std::ldexp( 1.0, -39 ) && acn_select_hist_edge( 2 ) == std::ldexp( 1.25, -40 ) );
    for( uint32_t j = 1; j < 256; j++ )
    {
        const double e = acn_select_hist_edge( j );
        uint64_t u; memcpy( &u, &e, 8 );
        EXPECT( acn_select_key_bin( u ) == j && acn_select_key_bin( u - 1 ) == j - 1 && acn_select_key_bin( u + 1 ) == j );
    }
    EXPECT( acn_select_key_bin( 0 ) == 0 && acn_select_key_bin( 0x8000000000000000ull ) == 0 && acn_select_key_bin( 0xFFF0000000000000ull ) == 0 );
    EXPECT( acn_select_key_bin( 0x7FF0000000000000ull ) == 255 && acn_select_key_bin( 0x7FF0000000000001ull ) == 256 && acn_select_key_bin( 0xFFF8000000000000ull ) == 256 );
    EXPECT( acn_select_key_bin( ~( uint64_t )0 ) == 256 && acn_select_key_bin( 1 ) == 0 && acn_select_key_bin( 0x7FEFFFFFFFFFFFFFull ) == 255 );
    {
        std::unique_ptr< uint64_t[] > hist( new uint64_t[ ACN_KEY_HIST_WORDS ] );
        for( int j = 0; j < ACN_KEY_HIST_WORDS; j++ ) hist[ j ] = 0;
        EXPECT( acn_select_hist_threshold( hist.get(), 0 ) == acn_select_hist_edge( 1 ) );
        hist[ 0 ] = 1000; hist[ 256 ] = 1000;                                  /* neither counts: below every edge, and NaN */
        EXPECT( acn_select_hist_threshold( hist.get(), 0 ) == acn_select_hist_edge( 1 ) );
        hist[ 255 ] = 5;
        EXPECT( acn_select_hist_threshold( hist.get(), 4 ) == inf && acn_select_hist_threshold( hist.get(), 5 ) == acn_select_hist_edge( 1 ) );
        hist[ 1 ] = 1;
        EXPECT( acn_select_hist_threshold( hist.get(), 5 ) == acn_select_hist_edge( 2 ) && acn_select_hist_threshold( hist.get(), 6 ) == acn_select_hist_edge( 1 ) );
        hist[ 255 ] = hist[ 254 ] = ~( uint64_t )0;                             /* a sum past 2^64 does not wrap: it is above every budget */
        EXPECT( acn_select_hist_threshold( hist.get(), ~( uint64_t )0 ) == acn_select_hist_edge( 255 ) );
        EXPECT( acn_select_hist_threshold( hist.get(), ~( uint64_t )0 - 1 ) == inf );
        EXPECT( std::isnan( acn_select_hist_threshold( nullptr, 1 ) ) );
    }
    EXPECT( acn_select_tiles( 0 ) == 0 && acn_select_tiles( 1 ) == 1 && acn_select_tiles( ACN_SELECT_TILE ) == 1 && acn_select_tiles( ACN_SELECT_TILE + 1 ) == 2 );
    EXPECT( acn_select_tiles( ACN_SELECT_MAX_N ) == ACN_SELECT_MAX_N / ACN_SELECT_TILE );

    if( failures ) { printf( "%d checks failed\n", failures ); return 1; }
    printf( "ok\n" );
    return 0;
}
#endif
