/* actinon_amd/csrc/acn_queueplan.h on its own, twice.  As a shared library it is the extern "C" shim through which
 * tests/test_queueplan_cpu.py compares the planning arithmetic of the pipeline runner with a Python model of each rule.  With
 * -DQUEUEPLAN_CPU_MAIN it is a program that the same test builds with -fsanitize=address,undefined and runs: every rule at its
 * edges, each array in a heap block of exactly its size, so a read past a queue's entry or a counter block is a sanitizer report
 * and an overflowing conversion an error.  The program prints "ok" and returns 0, or names what failed. */
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "acn_queueplan.h"

extern "C"
{
uint64_t qp_first_chunk_guess( uint32_t cap_children, uint32_t cap_hs, uint64_t ps, uint64_t ds, uint64_t n_lights, uint64_t most )
{ return acn_first_chunk_guess( cap_children, cap_hs, ps, ds, ( size_t )n_lights, ( size_t )most ); }
uint64_t qp_sample_positions( uint32_t cap_children, uint32_t cap_hs, uint64_t ps, uint64_t ds, uint64_t n_lights, uint64_t n )
{ return acn_sample_positions( cap_children, cap_hs, ps, ds, ( size_t )n_lights, ( size_t )n ); }
void qp_wanted_caps( const double* rate, int seeded, uint64_t n, uint64_t ps, uint64_t ds, uint64_t n_lights, uint64_t budget, uint64_t stack_bytes,
                     const uint64_t* rec_bytes, uint64_t* want )
{
    size_t rb[ WQ_N ], w[ WQ_N ];
    for( int q = 0; q < WQ_N; q++ ) rb[ q ] = ( size_t )rec_bytes[ q ];
    acn_wanted_caps( rate, seeded, ( size_t )n, ps, ds, ( size_t )n_lights, ( size_t )budget, ( size_t )stack_bytes, rb, w );
    for( int q = 0; q < WQ_N; q++ ) want[ q ] = w[ q ];
}
int qp_keep_caps( const uint32_t* cap, uint64_t have_waves, uint64_t waves, const uint64_t* want, const uint64_t* rec_bytes, int known, uint32_t rate_cnt,
                  int trimmed, uint32_t* sized_calls, int* trim )
{
    size_t rb[ WQ_N ], w[ WQ_N ];
    for( int q = 0; q < WQ_N; q++ ) { rb[ q ] = ( size_t )rec_bytes[ q ]; w[ q ] = ( size_t )want[ q ]; }
    return acn_keep_caps( cap, ( size_t )have_waves, ( size_t )waves, w, rb, known, rate_cnt, trimmed, sized_calls, trim );
}
int qp_halve_caps( uint64_t* want )
{
    size_t w[ WQ_N ];
    for( int q = 0; q < WQ_N; q++ ) w[ q ] = ( size_t )want[ q ];
    const int floor = acn_halve_caps( w );
    for( int q = 0; q < WQ_N; q++ ) want[ q ] = w[ q ];
    return floor;
}
int qp_rates_known( const double* rate ) { return acn_rates_known( rate ); }
double qp_queue_demand( const double* rate, int q, int seeded ) { return acn_queue_demand( rate, q, seeded ); }
uint64_t qp_chunk_for_caps( const double* rate, int seeded, double fill_target, const uint32_t* cap ) { return acn_chunk_for_caps( rate, seeded, fill_target, cap ); }
void qp_set_rates( double* rate, uint32_t* rate_cnt, uint32_t cnt, const uint32_t* fill, double dead_share ) { acn_set_rates( rate, rate_cnt, cnt, fill, dead_share ); }
void qp_learn_rates( double* rate, uint32_t* rate_cnt, uint32_t cnt, const uint32_t* fill, double dead_share ) { acn_learn_rates( rate, rate_cnt, cnt, fill, dead_share ); }
void qp_overflow_rates( double* rate, uint32_t cnt, const uint32_t* fill ) { acn_overflow_rates( rate, cnt, fill ); }
void qp_sample_rates( const uint32_t* counts, int levels, uint32_t cnt, uint64_t plan_positions, unsigned plan_grid, double* rate )
{ acn_sample_rates( counts, levels, cnt, ( size_t )plan_positions, plan_grid, rate ); }
/* acn_read_chunk; the report as words: flags, verdict, fill[ WQ_N ], passes_seen[ ACN_LEVEL_BLOCKS ], then the nine statistics in the order of the struct */
void qp_read_chunk( uint32_t* counts, int levels, const uint32_t* passes, int seeded, uint64_t* words, double* dead_share )
{
    acn_chunk_report r;
    acn_read_chunk( counts, levels, passes, seeded, &r );
    *words++ = r.flags; *words++ = ( uint64_t )r.verdict;
    for( int q = 0; q < WQ_N; q++ ) *words++ = r.fill[ q ];
    for( int level = 0; level < ACN_LEVEL_BLOCKS; level++ ) *words++ = r.passes_seen[ level ];
    for( uint64_t v : { r.levels, r.walk_rays, r.walk_steps, r.hard_rays, r.shade_hit_recs, r.private_rays, r.probe_rays, ( uint64_t )r.peak_tasks, ( uint64_t )r.peak_children } ) *words++ = v;
    *dead_share = r.dead_share;
}
/* a constant of acn_counts.h or acn_queueplan.h by its name; -1: not one of these */
int64_t qp_constant( const char* name )
{
#define K( x ) { #x, ( int64_t )( x ) }
    static const struct { const char* name; int64_t value; } known[] = {
        K( QC_TASKS ), K( QC_CLASS0 ), K( QC_CHILDREN ), K( QC_FLAGS ), K( QC_HARD_SHADOW ), K( QC_HARD_PATH ), K( QS_WALK_RAYS ), K( QS_HARD_SHADOW ),
        K( QS_HARD_PATH ), K( QS_CHILDREN ), K( QS_TASKS ), K( QS_WALK_STEPS ), K( QS_PRIVATE_RAYS ), K( QS_PROBES ), K( QS_DEAD_T ), K( QS_DEAD_C ),
        K( QS_DEAD_HP ), K( QS_DEAD_R ), K( QC_GEN ), K( QC_CUR_GEN ), K( QC_N ), K( ACN_QCHUNK ), K( ACN_NCLASS ), K( ACN_MAX_WALK_PASSES ),
        K( ACN_MAX_PATH_LEVELS ), K( ACN_LEVEL_BLOCKS ), K( ACN_FLAG_TASK_OVERFLOW ), K( ACN_FLAG_CHILD_OVERFLOW ), K( ACN_FLAG_STACK_OVERFLOW ),
        K( ACN_FLAG_CLAMPED ), K( ACN_FLAGS_CHUNK_LOST ), K( WQ_N ), K( ACN_CHUNK_FITS ), K( ACN_CHUNK_OVERFLOW ), K( ACN_CHUNK_STACK_OVERFLOW ) };
#undef K
    for( const auto& k : known ) if( !strcmp( k.name, name ) ) return k.value;
    return -1;
}
uint32_t qp_walk_passes( uint64_t trace_depth, int level, uint32_t tun_passes, uint32_t seen ) { return acn_walk_passes( trace_depth, level, tun_passes, seen ); }
uint32_t qp_walk_passes_seen( const uint32_t* gen, uint32_t launched ) { return acn_walk_passes_seen( gen, launched ); }
uint64_t qp_lane_count( uint64_t n, int lanes, int lane ) { return acn_lane_count( ( size_t )n, lanes, lane ); }
int qp_lanes_for_counts( int tun_lanes, uint64_t n, uint64_t ps ) { return acn_lanes_for_counts( tun_lanes, ( size_t )n, ps ); }
int qp_one_lane( const double* rate, int seeded, uint64_t n, const uint64_t* rec_bytes, uint64_t budget, int was_one_lane )
{
    size_t rb[ WQ_N ];
    for( int q = 0; q < WQ_N; q++ ) rb[ q ] = ( size_t )rec_bytes[ q ];
    return acn_one_lane( rate, seeded, ( size_t )n, rb, ( size_t )budget, was_one_lane );
}
uint32_t qp_tile_order( uint64_t n, int shift, uint32_t* mul ) { return acn_tile_order( ( size_t )n, shift, mul ); }
}

#ifdef QUEUEPLAN_CPU_MAIN
static int failures = 0;
#define EXPECT( cond ) do { if( !( cond ) ) { printf( "line %d: %s\n", __LINE__, #cond ); failures++; } } while( 0 )

/* `n` values in a heap block of exactly that size */
template< class T > static std::unique_ptr< T[] > block( std::initializer_list< T > v )
{
    std::unique_ptr< T[] > b( new T[ v.size() ] );
    size_t i = 0;
    for( T x : v ) b[ i++ ] = x;
    return b;
}

int main()
{
    /* the record sizes of the device structs do not matter here: five plausible ones */
    auto rb = block< size_t >( { 112, 48, 64, 96, 160 } );
    auto none = block< double >( { 0, 0, 0, 0, 0 } );
    auto want = block< size_t >( { 0, 0, 0, 0, 0 } );

    /* the first-chunk guess and the sample: path_samples 0, 16, 64, 1024 */
    const uint32_t cap = 1u << 20;
    for( uint64_t ps : { 0ull, 16ull, 64ull, 1024ull } )
    {
        const size_t g = acn_first_chunk_guess( cap, 2 * cap, ps, 50, 3, 32768 ), s = acn_sample_positions( cap, 2 * cap, ps, 50, 3, 57600 );
        EXPECT( g <= 32768 && s >= 256 && s <= 4096 );
        if( ps == 1024 ) EXPECT( acn_first_chunk_guess( cap, 2 * cap, ps, 50, 3, 4096 ) == 63 && s == 256 );
    }
    EXPECT( acn_sample_positions( cap, 2 * cap, 16, 50, 3, 100 ) == 25 && acn_sample_positions( cap, 2 * cap, 16, 50, 3, 0 ) == 0 );

    /* starter set: a budget smaller than the stacks gives the floor; n below 64 */
    acn_wanted_caps( none.get(), 0, 57600, 64, 50, 3, 1000, 2000, rb.get(), want.get() );
    for( int q = 0; q < WQ_N; q++ ) EXPECT( want[ q ] == 65536 );
    acn_wanted_caps( none.get(), 0, 5, 16, 50, 3, ( size_t )8 << 30, 1 << 20, rb.get(), want.get() );
    EXPECT( want[ WQ_TASKS ] == 5 * ( 18 + 150 ) + 65536 && want[ WQ_HARD_SHADOW ] == 2 * want[ WQ_TASKS ] );
    /* learned: a demand above 4e9 records is clamped; a ray call with a ray rate below 1 */
    auto huge = block< double >( { 1.0, 1e6, 1.0, 1.0, 0.25 } );
    acn_wanted_caps( huge.get(), 0, ( size_t )1 << 22, 64, 50, 3, ~( size_t )0, 0, rb.get(), want.get() );
    EXPECT( want[ WQ_CHILDREN ] == 0xFFFFFF00ull );
    acn_wanted_caps( huge.get(), 0, 100000, 64, 50, 3, 1000, 2000, rb.get(), want.get() );       /* no room at all: the floor */
    for( int q = 0; q < WQ_N; q++ ) EXPECT( want[ q ] == 65536 );
    EXPECT( acn_queue_demand( huge.get(), WQ_RAYS, 1 ) == 1.0 && acn_queue_demand( huge.get(), WQ_RAYS, 0 ) == 0.25 && acn_queue_demand( huge.get(), WQ_TASKS, 1 ) == 1.0 );
    auto caps = block< uint32_t >( { 100000, 100000, 100000, 100000, 100000 } );
    EXPECT( acn_chunk_for_caps( huge.get(), 1, 0.7, caps.get() ) == 64 && acn_chunk_for_caps( none.get(), 0, 0.7, caps.get() ) + 1 - 70000000 <= 1 );

    /* keep / trim with its window, and the halving */
    {
        auto big = block< uint32_t >( { 1u << 24, 1u << 24, 1u << 24, 1u << 24, 1u << 24 } );
        auto w = block< size_t >( { 1 << 20, 1 << 20, 1 << 20, 1 << 20, 1 << 20 } );
        uint32_t calls = 2; int trim = 0;
        EXPECT( acn_keep_caps( big.get(), 4096, 4096, w.get(), rb.get(), 1, 40000, 0, &calls, &trim ) == 0 && trim == 1 && calls == 3 );
        EXPECT( acn_keep_caps( big.get(), 4096, 4096, w.get(), rb.get(), 1, 40000, 0, &calls, &trim ) == 1 && trim == 0 && calls == 4 );
        EXPECT( acn_keep_caps( big.get(), 4095, 4096, w.get(), rb.get(), 0, 0, 0, &calls, &trim ) == 0 && trim == 0 && calls == 4 );
        EXPECT( acn_halve_caps( w.get() ) == 0 && w[ 0 ] == 1 << 19 );
        auto f = block< size_t >( { 65536, 65536, 65536, 65536, 65536 } );
        EXPECT( acn_halve_caps( f.get() ) == 1 && f[ 4 ] == 65536 );
    }
    /* rates */
    {
        auto rate = block< double >( { 0, 0, 0, 0, 0 } );
        auto fill = block< uint32_t >( { 4000, 0, 8000, 1, 0xFFFFFFFFu } );
        uint32_t rc = 0;
        acn_learn_rates( rate.get(), &rc, 1000, fill.get(), 0.5 );
        EXPECT( rc == 1000 && rate[ 0 ] == 2.0 && rate[ 1 ] == 1e-3 && acn_rates_known( rate.get() ) );
        acn_learn_rates( rate.get(), &rc, 2000, fill.get(), 0.5 );
        EXPECT( rc == 2000 && rate[ 0 ] == 2.0 && rate[ 2 ] == 4.0 );
        acn_overflow_rates( rate.get(), 1, fill.get() );
        EXPECT( rate[ 4 ] == 4294967295.0 );
    }
    /* the learning sample: two levels of counter words in a block of exactly their size */
    {
        std::unique_ptr< uint32_t[] > c( new uint32_t[ 2 * QC_N ] );
        for( int i = 0; i < 2 * QC_N; i++ ) c[ i ] = ( uint32_t )( i * 37 % 1000 );
        auto rate = block< double >( { 0, 0, 0, 0, 0 } );
        acn_sample_rates( c.get(), 2, 4096, 19200, 256, rate.get() );
        for( int q = 0; q < WQ_N; q++ ) EXPECT( rate[ q ] >= 1e-3 );
    }
    /* the reader of a chunk's counter blocks: every level the device has, every pass a level can get, in a block of exactly
     * levels * QC_N words -- QC_GEN + passes is then the last generation word of each level */
    {
        const int levels = ACN_LEVEL_BLOCKS;
        std::unique_ptr< uint32_t[] > c( new uint32_t[ ( size_t )levels * QC_N ] );
        std::unique_ptr< uint32_t[] > passes( new uint32_t[ levels ] );
        auto level = [ & ]( int l ) { return c.get() + ( size_t )l * QC_N; };
        auto clear = [ & ]() { memset( c.get(), 0, sizeof( uint32_t ) * levels * QC_N ); for( int l = 0; l < levels; l++ ) passes[ l ] = ACN_MAX_WALK_PASSES; };
        acn_chunk_report r;
        /* a chunk that fits: marks, statistics up to the first empty level, the seeded word cleared */
        clear();
        for( int l = 0; l < 3; l++ ) { level( l )[ QC_TASKS ] = 10 + l; level( l )[ QS_WALK_RAYS ] = 100; level( l )[ QS_WALK_STEPS ] = 7; level( l )[ QC_GEN + 1 ] = 50 + l; }
        level( 4 )[ QC_TASKS ] = 999; level( 4 )[ QS_WALK_RAYS ] = 5;    /* behind the empty level 3: in the marks, not in the statistics */
        level( 0 )[ QC_GEN + 0 ] = 4000; level( 0 )[ QC_FLAGS ] = ACN_FLAG_CLAMPED;
        level( 1 )[ QC_CLASS0 + 3 ] = 2000;
        acn_read_chunk( c.get(), levels, passes.get(), 1, &r );
        EXPECT( r.verdict == ACN_CHUNK_FITS && r.flags == ACN_FLAG_CLAMPED && level( 0 )[ QC_GEN ] == 0 );
        EXPECT( r.fill[ WQ_TASKS ] == 2000 && r.fill[ WQ_RAYS ] == 52 && r.fill[ WQ_CHILDREN ] == 0 && r.dead_share == 0 );
        EXPECT( r.levels == 3 && r.walk_rays == 300 && r.walk_steps == 21 && r.peak_tasks == 12 );
        EXPECT( r.passes_seen[ 0 ] == 2 && r.passes_seen[ 2 ] == 2 && r.passes_seen[ 3 ] == 1 && r.passes_seen[ 5 ] == 1 );
        /* rays left in the last generation word of the last level, no flag anywhere: overflow, and no statistics */
        level( levels - 1 )[ QC_GEN + ACN_MAX_WALK_PASSES ] = 1;
        acn_read_chunk( c.get(), levels, passes.get(), 0, &r );
        EXPECT( r.verdict == ACN_CHUNK_OVERFLOW && r.flags == ( ACN_FLAG_CLAMPED | ACN_FLAG_CHILD_OVERFLOW ) && r.levels == 0 && r.passes_seen[ 0 ] == 0 && r.fill[ WQ_TASKS ] == 2000 );
        /* a stack overflow alone fails the call; together with a task overflow in a middle level the chunk is redone */
        clear();
        level( 2 )[ QC_FLAGS ] = ACN_FLAG_STACK_OVERFLOW;
        acn_read_chunk( c.get(), levels, passes.get(), 0, &r );
        EXPECT( r.verdict == ACN_CHUNK_STACK_OVERFLOW );
        level( 3 )[ QC_FLAGS ] = ACN_FLAG_TASK_OVERFLOW;
        acn_read_chunk( c.get(), levels, passes.get(), 0, &r );
        EXPECT( r.verdict == ACN_CHUNK_OVERFLOW && r.flags == ( ACN_FLAG_STACK_OVERFLOW | ACN_FLAG_TASK_OVERFLOW ) );
        /* the dead share: the fullest deferred-shadow mark is the last level's; records equal to the mark, then one below */
        clear();
        level( 0 )[ QC_HARD_SHADOW ] = 400; level( 0 )[ QS_HARD_SHADOW ] = 100;
        level( levels - 1 )[ QC_HARD_SHADOW ] = 1000; level( levels - 1 )[ QS_HARD_SHADOW ] = 600; level( levels - 1 )[ QS_PROBES ] = 400;
        acn_read_chunk( c.get(), levels, passes.get(), 0, &r );
        EXPECT( r.dead_share == 0 && r.fill[ WQ_HARD_SHADOW ] == 1000 );
        level( levels - 1 )[ QS_PROBES ] = 399;
        acn_read_chunk( c.get(), levels, passes.get(), 0, &r );
        EXPECT( r.dead_share == 1.0 / 1000.0 );
        /* every word at its largest */
        memset( c.get(), 0xFF, sizeof( uint32_t ) * levels * QC_N );
        for( int l = 0; l < levels; l++ ) level( l )[ QC_FLAGS ] = 0, level( l )[ QC_GEN + ACN_MAX_WALK_PASSES ] = 0;
        acn_read_chunk( c.get(), levels, passes.get(), 0, &r );
        EXPECT( r.verdict == ACN_CHUNK_FITS && r.levels == ( uint64_t )levels && r.hard_rays == 2ull * levels * 0xFFFFFFFFull && r.passes_seen[ 0 ] == ACN_MAX_WALK_PASSES + 2 );   /* (the last launch had input: two more) */
    }
    /* walk passes */
    EXPECT( acn_walk_passes( 10, 0, 4, 0 ) == 4 && acn_walk_passes( 10, 1, 4, 0 ) == 2 && acn_walk_passes( 2, 0, 4, 0 ) == 3 && acn_walk_passes( 50, 0, 32, 1 ) == 2 );
    EXPECT( acn_walk_passes( 50, 0, 4, 3 ) == 4 && acn_walk_passes( ~0ull - 1, 5, 32, 0 ) == 32 );
    {
        auto gen = block< uint32_t >( { 5, 0, 7, 0 } );
        EXPECT( acn_walk_passes_seen( gen.get(), 4 ) == 3 && acn_walk_passes_seen( gen.get(), 3 ) == 5 && acn_walk_passes_seen( gen.get(), 1 ) == 1 );
        EXPECT( acn_walk_passes_seen( gen.get() + 3, 1 ) == 1 && acn_walk_passes_seen( gen.get(), 0 ) == 1 );
    }
    /* lanes: the shares add up, also with a short last tile on every lane */
    for( int lanes = 1; lanes <= 16; lanes++ )
        for( size_t n : { ( size_t )0, ( size_t )1, ( size_t )255, ( size_t )256, ( size_t )257, ( size_t )57600, ( size_t )0xFFFFFF00ull } )
            for( int tiles = 0; tiles <= lanes; tiles++ )
            {
                const size_t m = n + ( size_t )tiles * 256;
                size_t sum = 0;
                for( int k = 0; k < lanes; k++ ) sum += acn_lane_count( m, lanes, k );
                EXPECT( sum == m );
            }
    EXPECT( acn_lanes_for_counts( 4, 57600, 16 ) == 1 && acn_lanes_for_counts( 4, 57600, 64 ) == 3 && acn_lanes_for_counts( 16, 0, 0 ) == 1 );
    EXPECT( acn_lanes_for_counts( 6, 0xFFFFFF00ull, 1024 ) == 6 );
    EXPECT( acn_one_lane( huge.get(), 0, 100, rb.get(), ( size_t )1 << 30, 0 ) == 1 && acn_one_lane( none.get(), 0, 100, rb.get(), 0, 1 ) == 0 );
    /* the order of work */
    for( size_t n : { ( size_t )0, ( size_t )1, ( size_t )512, ( size_t )513, ( size_t )57600, ( size_t )0xFFFFFF00ull } )
    {
        uint32_t mul = 0;
        const uint32_t tiles = acn_tile_order( n, 8, &mul );
        EXPECT( tiles == ( n + 255 ) / 256 && ( tiles > 2 ? mul >= 1 && mul < tiles : mul == 1 ) );
    }
    if( failures ) { printf( "%d checks failed\n", failures ); return 1; }
    printf( "ok\n" );
    return 0;
}
#endif
