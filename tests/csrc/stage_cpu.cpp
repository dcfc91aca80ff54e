/* actinon_amd/csrc/acn_stage_host.h on its own: a program that tests/test_stages_cpu.py builds with -fsanitize=address,undefined and
 * runs.  Every refusal of acn_stage_plan / acn_run_stage and the capacities of an accepted call, with the records and the index list
 * in heap blocks of exactly their size, so a read past record n - 1 or index entry n_index - 1 is a sanitizer report.  The program
 * prints "ok" and returns 0, or names what failed. */
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "acn_stage_host.h"

static int failures = 0;
#define EXPECT( cond ) do { if( !( cond ) ) { printf( "line %d: %s\n", __LINE__, #cond ); failures++; } } while( 0 )
static bool says( const std::string& msg, const char* word ) { return msg.find( word ) != std::string::npos; }

static acn_stage_hitrec hit( uint32_t pixel, int depth = 12, int exit_obj = -1, int enter_obj = 0 )
{
    acn_stage_hitrec r;
    memset( &r, 0, sizeof( r ) );
    r.d.z = 1; r.intensity = 1; r.exit_obj = exit_obj; r.enter_obj = enter_obj; r.depth = depth; r.pixel = pixel;
    return r;
}
static acn_stage_dtask task( uint32_t pixel, double diffuse_intensity = 1.0, int depth = 12 )
{
    acn_stage_dtask t;
    memset( &t, 0, sizeof( t ) );
    t.surface_d.z = 1; t.diffuse_intensity = diffuse_intensity; t.depth = depth; t.pixel = pixel;
    return t;
}

int main()
{
    static_assert( sizeof( acn_stage_hitrec ) == 128 && sizeof( acn_stage_dtask ) == 144, "record sizes: DESIGN.md section 3" );
    const acn_stage_scene sc = { 7u, 2u, 50u, 16u };
    std::string msg;
    acn_stage_caps caps;
    const double inf = std::numeric_limits< double >::infinity(), nan = std::nan( "" );

    /* ---- the split ---- */
    {
        std::vector< acn_stage_hitrec > r;
        for( uint32_t i = 0; i < 5; i++ ) r.push_back( hit( i ) );
        r[ 3 ].pixel = ACN_STAGE_DEAD; r[ 3 ].depth = -7; r[ 3 ].enter_obj = 99;       /* a dead slot is not read further */
        r[ 4 ].enter_obj = 6; r[ 4 ].exit_obj = -1; r[ 4 ].depth = ACN_STAGE_MAX_DEPTH; r[ 4 ].pixel = 4;
        acn_stage_args a;
        memset( &a, 0, sizeof( a ) );
        a.stage = ACN_STAGE_SHADE_HITS; a.n = 5; a.in = r.data();
        EXPECT( acn_stage_check( true, &a, sc, &caps, &msg ) == ACN_OK );
        EXPECT( caps.grid == 2 && caps.chunk == 64 && caps.cap_children == 5 && caps.cap_hard_path == 0 );
        EXPECT( caps.cap_tasks == 5 + 2 * 4 * 64 && caps.cap_rays == 15 + 2 * 4 * 64 && caps.cap_hard_shadow == 15 + 2 * 4 * 64 );
        EXPECT( acn_stage_check( false, &a, sc, &caps, &msg ) == ACN_ERR_ARG && says( msg, "handle" ) );
        EXPECT( acn_stage_check( true, nullptr, sc, &caps, &msg ) == ACN_ERR_ARG && says( msg, "null" ) );
        EXPECT( acn_stage_check( true, &a, sc, nullptr, &msg ) == ACN_ERR_ARG && says( msg, "null" ) );
        { acn_stage_args b = a; b.stage = ACN_STAGE_N; EXPECT( acn_stage_check( true, &b, sc, &caps, &msg ) == ACN_ERR_ARG && says( msg, "stage" ) ); }
        { acn_stage_args b = a; b.flags = 8; EXPECT( acn_stage_check( true, &b, sc, &caps, &msg ) == ACN_ERR_ARG && says( msg, "flags" ) ); }
        { acn_stage_args b = a; b.flags = 7; EXPECT( acn_stage_check( true, &b, sc, &caps, &msg ) == ACN_OK ); }
        /* bit 16, ACN_STAGE_COUNT_WORK: the counting variants, alone and beside the others; the walk's bit 8 stays refused beside it, and bit 32 is unknown */
        { acn_stage_args b = a; b.flags = ACN_STAGE_COUNT_WORK; EXPECT( ACN_STAGE_COUNT_WORK == 16u && acn_stage_check( true, &b, sc, &caps, &msg ) == ACN_OK ); }
        { acn_stage_args b = a; b.flags = 7 | ACN_STAGE_COUNT_WORK; EXPECT( acn_stage_check( true, &b, sc, &caps, &msg ) == ACN_OK ); }
        { acn_stage_args b = a; b.flags = 8 | ACN_STAGE_COUNT_WORK; EXPECT( acn_stage_check( true, &b, sc, &caps, &msg ) == ACN_ERR_ARG && says( msg, "flags" ) ); }
        { acn_stage_args b = a; b.flags = 32; EXPECT( acn_stage_check( true, &b, sc, &caps, &msg ) == ACN_ERR_ARG && says( msg, "flags" ) ); }
        { acn_stage_args b = a; b.in = nullptr; EXPECT( acn_stage_check( true, &b, sc, &caps, &msg ) == ACN_ERR_ARG && says( msg, "in" ) ); }
        { acn_stage_args b = a; b.n = 0; EXPECT( acn_stage_check( true, &b, sc, &caps, &msg ) == ACN_ERR_ARG && says( msg, "records" ) ); }
        { acn_stage_args b = a; b.n = ACN_STAGE_MAX_RECORDS + 1; EXPECT( acn_stage_check( true, &b, sc, &caps, &msg ) == ACN_ERR_ARG && says( msg, "records" ) ); }
        auto refused = [ & ]( acn_stage_hitrec bad, const char* word )
        {
            std::vector< acn_stage_hitrec > q = r;
            q[ 4 ] = bad;                                                          /* the last record: the loop reaches the end of the block */
            acn_stage_args b = a; b.in = q.data();
            msg.clear();
            return acn_stage_check( true, &b, sc, &caps, &msg ) == ACN_ERR_ARG && says( msg, word ) && says( msg, "hit record 4" );
        };
        EXPECT( refused( hit( 5 ), "pixel" ) );
        EXPECT( refused( hit( 0xFFFFFFFEu ), "pixel" ) );
        EXPECT( refused( hit( 4, -1 ), "depth" ) );
        EXPECT( refused( hit( 4, ACN_STAGE_MAX_DEPTH + 1 ), "depth" ) );
        EXPECT( refused( hit( 4, 12, 7 ), "object" ) );
        EXPECT( refused( hit( 4, 12, -2 ), "object" ) );
        EXPECT( refused( hit( 4, 12, -1, 7 ), "object" ) );
        EXPECT( refused( hit( 4, 12, 0, std::numeric_limits< int >::min() ), "object" ) );
        /* the reservation of k_shade_hits grows with the input (chunks_resize) */
        EXPECT( acn_stage_chunk( ACN_STAGE_SHADE_HITS, 1u << 20, 64 ) == 512 && acn_stage_chunk( ACN_STAGE_SHADE_HITS, 256 * 8 * 64 * 2, 64 ) == 128 );
        EXPECT( acn_stage_chunk( ACN_STAGE_SHADE_HITS, 2000, 64 ) == 64 && acn_stage_chunk( ACN_STAGE_SHADE, 1u << 20, 64 ) == 64 );
    }

    /* ---- the sample loops ---- */
    {
        std::vector< acn_stage_dtask > t;
        for( uint32_t i = 0; i < 4; i++ ) t.push_back( task( i ) );
        t[ 1 ].diffuse_intensity = 0.001;     /* one sample of each loop */
        t[ 2 ].depth = 10;                    /* no path loop */
        t[ 3 ] = task( 77, nan, -5 );         /* never listed: not read */
        std::vector< uint32_t > ix = { 0, 1, ACN_STAGE_DEAD, 2, 0 };
        acn_stage_args a;
        memset( &a, 0, sizeof( a ) );
        a.stage = ACN_STAGE_SHADE; a.n = 4; a.in = t.data(); a.index = ix.data(); a.n_index = 5; a.cls = 3;
        EXPECT( acn_stage_check( true, &a, sc, &caps, &msg ) == ACN_OK );
        /* direct: ( 50 + 1 + 50 + 50 ) * 2 lights; path: 16 + 1 + 0 + 16 */
        EXPECT( caps.grid == 2 && caps.chunk == 64 && caps.cap_tasks == 5 && caps.cap_rays == 0 );
        EXPECT( caps.cap_children == 33 + 512 && caps.cap_hard_path == 33 + 512 && caps.cap_hard_shadow == 302 + 33 + 512 );
        { acn_stage_args b = a; b.cls = 4; EXPECT( acn_stage_check( true, &b, sc, &caps, &msg ) == ACN_ERR_ARG && says( msg, "class" ) ); }
        { acn_stage_args b = a; b.shard_world = 3; b.shard_rank = 3; EXPECT( acn_stage_check( true, &b, sc, &caps, &msg ) == ACN_ERR_ARG && says( msg, "shard" ) ); }
        { acn_stage_args b = a; b.shard_world = 3; b.shard_rank = 2; EXPECT( acn_stage_check( true, &b, sc, &caps, &msg ) == ACN_OK ); }
        { acn_stage_args b = a; b.shard_world = 0; b.shard_rank = 1; EXPECT( acn_stage_check( true, &b, sc, &caps, &msg ) == ACN_ERR_ARG && says( msg, "shard" ) ); }
        { acn_stage_args b = a; b.index = nullptr; EXPECT( acn_stage_check( true, &b, sc, &caps, &msg ) == ACN_ERR_ARG && says( msg, "index" ) ); }
        { acn_stage_args b = a; b.n_index = 0; EXPECT( acn_stage_check( true, &b, sc, &caps, &msg ) == ACN_ERR_ARG && says( msg, "n_index" ) ); }
        { acn_stage_args b = a; b.n_index = ACN_STAGE_MAX_RECORDS + 1; EXPECT( acn_stage_check( true, &b, sc, &caps, &msg ) == ACN_ERR_ARG && says( msg, "n_index" ) ); }
        { std::vector< uint32_t > jx = ix; jx[ 4 ] = 4; acn_stage_args b = a; b.index = jx.data();
          EXPECT( acn_stage_check( true, &b, sc, &caps, &msg ) == ACN_ERR_ARG && says( msg, "index entry 4" ) ); }
        auto refused = [ & ]( acn_stage_dtask bad, const char* word )
        {
            std::vector< acn_stage_dtask > q = t;
            q[ 2 ] = bad;
            acn_stage_args b = a; b.in = q.data();
            msg.clear();
            return acn_stage_check( true, &b, sc, &caps, &msg ) == ACN_ERR_ARG && says( msg, word ) && says( msg, "task 2" );
        };
        EXPECT( refused( task( 4 ), "pixel" ) );
        EXPECT( refused( task( ACN_STAGE_DEAD ), "pixel" ) );
        EXPECT( refused( task( 2, 1.0, -1 ), "depth" ) );
        EXPECT( refused( task( 2, 1.0, ACN_STAGE_MAX_DEPTH + 1 ), "depth" ) );
        EXPECT( refused( task( 2, nan ), "diffuse_intensity" ) );
        EXPECT( refused( task( 2, inf ), "diffuse_intensity" ) );
        EXPECT( refused( task( 2, -1e-300 ), "diffuse_intensity" ) );
        EXPECT( refused( task( 2, 65538.0 / 50.0 ), "diffuse_intensity" ) );         /* 65538 direct samples */
        EXPECT( refused( task( 2, 5000.0, 12 ), "diffuse_intensity" ) );             /* 80000 path samples */
        EXPECT( !refused( task( 2, 1300.0, 10 ), "diffuse_intensity" ) && msg.empty() );   /* 65000 direct samples, no path loop */
        /* the sample counts as the kernels count them */
        bool ok = true;
        EXPECT( acn_stage_samples( 50, 0.0, &ok ) == 1 && acn_stage_samples( 50, 0.019, &ok ) == 1 && acn_stage_samples( 50, 0.04, &ok ) == 2 && ok );
        EXPECT( acn_stage_samples( 50, 0.9999999999999999, &ok ) == 49 && acn_stage_samples( 1u << 16, 1.0, &ok ) == 1u << 16 && ok );
        /* a queue above 2^26 records is refused, not wrapped */
        {
            const acn_stage_scene big = { 7u, 4096u, 1u << 16, 0u };
            std::vector< acn_stage_dtask > q( 1, task( 0 ) );
            std::vector< uint32_t > jx( 1, 0u );
            acn_stage_args b = a; b.n = 1; b.in = q.data(); b.index = jx.data(); b.n_index = 1;
            EXPECT( acn_stage_check( true, &b, big, &caps, &msg ) == ACN_ERR_ARG && says( msg, "2^26" ) );
        }
    }

    if( failures ) { printf( "%d checks failed\n", failures ); return 1; }
    printf( "ok\n" );
    return 0;
}
