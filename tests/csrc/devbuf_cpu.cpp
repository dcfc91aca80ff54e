/* devbuf_cpu.cpp -- the owning types of actinon_amd/csrc/acn_devbuf.h on a counting allocator over malloc, as a stand-alone program
 * for the address and undefined-behaviour sanitizers (tests/test_devbuf_cpu.py): what the types lose, the leak check sees; what they
 * free twice, the address check does.  Every call of the policy is logged, and the k-th allocation can be told to fail. */
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "acn_devbuf.h"

struct Op { char what; void* p; size_t bytes; };   /* 'a' allocated, 'x' an allocation that failed, 'f' freed */
static std::vector< Op > g_log;
static int g_allocs = 0, g_fail_at = 0;            /* g_fail_at: the allocation (counted from 1) that fails; 0: none */

struct Counting
{
    static int alloc( void** p, size_t want )
    {
        if( ++g_allocs == g_fail_at ) { *p = ( void* )16; g_log.push_back( { 'x', nullptr, want } ); return 2; }   /* (what it leaves in *p must not be kept) */
        *p = malloc( want );
        g_log.push_back( { 'a', *p, want } );
        return 0;
    }
    static void release( void* p ) { g_log.push_back( { 'f', p, 0 } ); free( p ); }
};
static void start( int fail_at ) { g_log.clear(); g_allocs = 0; g_fail_at = fail_at; }
static size_t count( char what, size_t from = 0 ) { size_t n = 0; for( size_t i = from; i < g_log.size(); i++ ) n += g_log[ i ].what == what; return n; }
static size_t freed( const void* p ) { size_t n = 0; for( const Op& o : g_log ) n += o.what == 'f' && o.p == p; return n; }

/* an object behind a handle: the index of its entry in g_destroyed, plus 1 (0: none) */
static std::vector< int > g_destroyed;
struct Slot { static void destroy( int h ) { g_destroyed[ h - 1 ]++; } };
static int make_slot( int* out ) { g_destroyed.push_back( 0 ); *out = ( int )g_destroyed.size(); return 0; }

#define CHECK( c ) do { if( !( c ) ) { printf( "line %d: %s\n", __LINE__, #c ); return 1; } } while( 0 )
typedef Buf< double, Counting > B;

/* the queues of a pipeline run as ensure_workspace allocates them: eleven blocks in order, released whole */
struct Eleven
{
    B q[ 11 ];
    void release() { for( B& b : q ) b.reset(); }
    int allocate( const size_t* bytes ) { int st = 0; for( int k = 0; k < 11 && st == 0; k++ ) st = q[ k ].grow( bytes[ k ] ); return st; }
};

static int checks()
{
    {   /* grow within the capacity, a larger grow, reset, the destructor */
        start( 0 );
        B b;
        CHECK( b.get() == nullptr && b.bytes() == 0 );
        CHECK( b.grow( 0 ) == 0 && g_log.empty() );
        CHECK( b.grow( 100 ) == 0 && b.get() && b.bytes() == 100 && g_log.size() == 1 );
        b.get()[ 0 ] = 1.0; b.get()[ 11 ] = 2.0;
        void* first = b.get();
        CHECK( b.grow( 100 ) == 0 && b.grow( 8 ) == 0 && b.grow( 0 ) == 0 && g_log.size() == 1 && b.get() == first );
        CHECK( b.grow( 101 ) == 0 && b.bytes() == 101 && g_log.size() == 3 );
        CHECK( g_log[ 1 ].what == 'f' && g_log[ 1 ].p == first && g_log[ 2 ].what == 'a' && g_log[ 2 ].bytes == 101 );   /* freed, THEN allocated */
        void* second = b.get();
        b.reset();
        CHECK( b.get() == nullptr && b.bytes() == 0 && freed( second ) == 1 );
        b.reset();
        CHECK( g_log.size() == 4 );
        CHECK( b.grow( 16 ) == 0 );
    }
    CHECK( g_log.size() == 6 && g_log[ 5 ].what == 'f' && g_log[ 5 ].p == g_log[ 4 ].p );   /* the destructor */
    {   /* an allocation that fails */
        start( 2 );
        {
            B b;
            CHECK( b.grow( 64 ) == 0 );
            void* first = b.get();
            CHECK( b.grow( 128 ) == 2 && b.get() == nullptr && b.bytes() == 0 );
            CHECK( g_log.size() == 3 && g_log[ 1 ].what == 'f' && g_log[ 1 ].p == first && g_log[ 2 ].what == 'x' );
        }
        CHECK( g_log.size() == 3 );   /* the destructor of a failed buffer frees nothing */
        start( 1 );
        B b;
        CHECK( b.grow( 32 ) == 2 && !b.get() && b.bytes() == 0 );
        CHECK( b.grow( 32 ) == 0 && b.get() && b.bytes() == 32 );   /* a later grow works */
        b.get()[ 3 ] = 4.0;
    }
    CHECK( count( 'a' ) == 1 && count( 'f' ) == 1 && count( 'x' ) == 1 );
    {   /* moves */
        start( 0 );
        void *pa, *pb, *pc;
        {
            B a, b2, c;
            CHECK( a.grow( 24 ) == 0 && b2.grow( 40 ) == 0 && c.grow( 56 ) == 0 );
            pa = a.get(); pb = b2.get(); pc = c.get();
            B m( std::move( a ) );
            CHECK( a.get() == nullptr && a.bytes() == 0 && m.get() == pa && m.bytes() == 24 && count( 'f' ) == 0 );
            b2 = std::move( m );   /* over a live buffer: its block goes now */
            CHECK( m.get() == nullptr && m.bytes() == 0 && b2.get() == pa && b2.bytes() == 24 && freed( pb ) == 1 && count( 'f' ) == 1 );
            B& self = b2;
            b2 = std::move( self );
            CHECK( b2.get() == pa && count( 'f' ) == 1 );
            c.reset();
            CHECK( freed( pc ) == 1 );
            std::vector< B > v;
            v.push_back( std::move( b2 ) );
            for( int k = 0; k < 9; k++ ) v.emplace_back();   /* the vector moves its elements as it grows */
            CHECK( v[ 0 ].get() == pa && count( 'f' ) == 2 );
        }
        CHECK( freed( pa ) == 1 && freed( pb ) == 1 && freed( pc ) == 1 && count( 'f' ) == 3 && count( 'a' ) == 3 );
    }
    {   /* ensure_workspace: eleven buffers in order, allocation 7 fails, released whole, halved, allocated again */
        start( 7 );
        size_t bytes[ 11 ];
        for( int k = 0; k < 11; k++ ) bytes[ k ] = 1000 + 8 * ( size_t )k;
        std::vector< void* > round1, round2;
        {
            Eleven w;
            CHECK( w.allocate( bytes ) == 2 );
            CHECK( g_log.size() == 7 && count( 'a' ) == 6 && g_log[ 6 ].what == 'x' && g_log[ 6 ].bytes == bytes[ 6 ] );
            for( int k = 0; k < 11; k++ ) { CHECK( ( w.q[ k ].get() != nullptr ) == ( k < 6 ) ); if( k < 6 ) { CHECK( g_log[ k ].bytes == bytes[ k ] ); round1.push_back( w.q[ k ].get() ); } }
            w.release();
            for( int k = 0; k < 11; k++ ) CHECK( w.q[ k ].get() == nullptr && w.q[ k ].bytes() == 0 );
            CHECK( count( 'f' ) == 6 );
            for( int k = 0; k < 6; k++ ) CHECK( g_log[ 7 + k ].what == 'f' && g_log[ 7 + k ].p == round1[ k ] );
            for( size_t& b : bytes ) b /= 2;
            const size_t before = g_log.size();
            CHECK( w.allocate( bytes ) == 0 && g_log.size() == before + 11 && count( 'a', before ) == 11 );
            for( int k = 0; k < 11; k++ ) { CHECK( w.q[ k ].get() && w.q[ k ].bytes() == bytes[ k ] && g_log[ before + k ].bytes == bytes[ k ] ); round2.push_back( w.q[ k ].get() ); }
            CHECK( count( 'f' ) == 6 );
        }
        CHECK( count( 'f' ) == 17 && count( 'a' ) == 17 );   /* (malloc may hand a block of round 1 out again in round 2: the totals say once each) */
        for( void* p : round2 ) CHECK( freed( p ) >= 1 );
    }
    {   /* the owners of an event and of a stream */
        typedef Owned< int, Slot > O;
        {
            O a;
            CHECK( a.get() == 0 );
            CHECK( make_slot( a.put() ) == 0 && a.get() == 1 );
            O m( std::move( a ) );
            CHECK( a.get() == 0 && m.get() == 1 && g_destroyed[ 0 ] == 0 );
            O b2;
            make_slot( b2.put() );
            b2 = std::move( m );   /* over a live one */
            CHECK( m.get() == 0 && b2.get() == 1 && g_destroyed[ 1 ] == 1 && g_destroyed[ 0 ] == 0 );
            std::vector< O > v;
            v.push_back( std::move( b2 ) );
            for( int k = 0; k < 9; k++ ) v.emplace_back();
            CHECK( v[ 0 ].get() == 1 && g_destroyed[ 0 ] == 0 );
            make_slot( v[ 1 ].put() );
            make_slot( v[ 1 ].put() );   /* made again in place: the old one goes first */
            CHECK( g_destroyed[ 2 ] == 1 && g_destroyed[ 3 ] == 0 );
            v[ 1 ].reset(); v[ 1 ].reset();
            CHECK( g_destroyed[ 3 ] == 1 );
        }
        CHECK( g_destroyed.size() == 4 );
        for( int d : g_destroyed ) CHECK( d == 1 );
    }
    return 0;
}

int main()
{
    if( checks() ) return 1;
    printf( "ok\n" );
    return 0;
}
