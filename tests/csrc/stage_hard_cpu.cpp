/* actinon_amd/csrc/acn_stage_host.h on its own, the two hard-ray stages (ACN_STAGE_HARD_SHADOW, ACN_STAGE_HARD_PATH): a program that
 * tests/test_stages_hard_cpu.py builds with -fsanitize=address,undefined and runs.  Every refusal of the two stages and the plan of an
 * accepted call, with the records in heap blocks of exactly their size, so a read past record n - 1 is a sanitizer report.  The program
 * prints "ok" and returns 0, or names what failed. */
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "acn_stage_host.h"

static int failures = 0;
#define EXPECT( cond ) do { if( !( cond ) ) { printf( "line %d: %s\n", __LINE__, #cond ); failures++; } } while( 0 )
static bool says( const std::string& msg, const char* word ) { return msg.find( word ) != std::string::npos; }

static acn_stage_hardshadow shadow( uint32_t pixel, uint32_t pad = 1u, double limit = 2.5 )
{
    acn_stage_hardshadow r;
    memset( &r, 0, sizeof( r ) );
    r.d.z = 1; r.limit = limit; r.contrib.x = 0.5; r.pixel = pixel; r.pad = pad;
    return r;
}
static acn_stage_hardpath path( uint32_t pixel, uint32_t resume = 6u, int depth = 2 )
{
    acn_stage_hardpath r;
    memset( &r, 0, sizeof( r ) );
    r.d.z = 1; r.T.x = 1; r.intensity = 0.5; r.depth = depth; r.pixel = pixel; r.resume = resume;
    return r;
}

int main()
{
    static_assert( sizeof( acn_stage_hardshadow ) == 88 && sizeof( acn_stage_hardpath ) == 96, "record sizes: DESIGN.md section 3" );
    const acn_stage_scene sc = { 7u, 2u, 50u, 16u };
    std::string msg;
    acn_stage_caps caps;
    const double inf = std::numeric_limits< double >::infinity(), nan = std::nan( "" );

    /* ---- k_hard_shadow ---- */
    {
        std::vector< acn_stage_hardshadow > r;
        for( uint32_t i = 0; i < 6; i++ ) r.push_back( shadow( i ) );
        r[ 1 ].pad = 0;                                   /* nothing known, the matter root alone */
        r[ 2 ].pad = ( 5u << 2 ) | 2u;                    /* a resume word */
        r[ 3 ] = shadow( ACN_STAGE_DEAD, 3u, nan );       /* a dead slot is not read further */
        r[ 3 ].pos.x = nan;
        r[ 4 ].limit = 1.7976931348623157e308;            /* a probe's "any finite hit" */
        r[ 5 ].pad = 2u;                                  /* a resume word without candidates */
        acn_stage_args a;
        memset( &a, 0, sizeof( a ) );
        a.stage = ACN_STAGE_HARD_SHADOW; a.n = 6; a.in = r.data();
        EXPECT( acn_stage_check( true, &a, sc, &caps, &msg ) == ACN_OK );
        EXPECT( caps.grid == 1 && caps.chunk == 64 && caps.cap_hard_shadow == 6 );
        EXPECT( caps.cap_tasks == 0 && caps.cap_rays == 0 && caps.cap_children == 0 && caps.cap_hard_path == 0 );
        EXPECT( acn_stage_check( false, &a, sc, &caps, &msg ) == ACN_ERR_ARG && says( msg, "handle" ) );
        { acn_stage_args b = a; b.in = nullptr; EXPECT( acn_stage_check( true, &b, sc, &caps, &msg ) == ACN_ERR_ARG && says( msg, "in" ) ); }
        { acn_stage_args b = a; b.n = 0; EXPECT( acn_stage_check( true, &b, sc, &caps, &msg ) == ACN_ERR_ARG && says( msg, "records" ) ); }
        { acn_stage_args b = a; b.flags = 8; EXPECT( acn_stage_check( true, &b, sc, &caps, &msg ) == ACN_ERR_ARG && says( msg, "flags" ) ); }
        /* the workgroups of the launch: by n, or as asked */
        { acn_stage_args b = a; b.cls = 64; EXPECT( acn_stage_check( true, &b, sc, &caps, &msg ) == ACN_OK && caps.grid == 64 ); }
        { acn_stage_args b = a; b.cls = 65; EXPECT( acn_stage_check( true, &b, sc, &caps, &msg ) == ACN_ERR_ARG && says( msg, "workgroups" ) ); }
        auto refused = [ & ]( acn_stage_hardshadow bad, const char* word )
        {
            std::vector< acn_stage_hardshadow > q = r;
            q[ 5 ] = bad;                                                          /* the last record: the loop reaches the end of the block */
            acn_stage_args b = a; b.in = q.data();
            msg.clear();
            return acn_stage_check( true, &b, sc, &caps, &msg ) == ACN_ERR_ARG && says( msg, word ) && says( msg, "hard-shadow record 5" );
        };
        EXPECT( refused( shadow( 6 ), "pixel" ) );
        EXPECT( refused( shadow( 0xFFFFFFFEu ), "pixel" ) );
        EXPECT( refused( shadow( 5, 1u, 0.0 ), "limit" ) );
        EXPECT( refused( shadow( 5, 1u, -1.0 ), "limit" ) );
        EXPECT( refused( shadow( 5, 1u, nan ), "limit" ) );
        EXPECT( !refused( shadow( 5, 1u, inf ), "limit" ) && msg.empty() );
        EXPECT( refused( shadow( 5, 3u ), "bit 0" ) );                              /* a probe carries no resume word */
        EXPECT( refused( shadow( 5, ( 1u << 2 ) | 3u ), "bit 0" ) );
        EXPECT( refused( shadow( 5, 4u ), "resume flag" ) );                        /* candidates without the flag */
        { acn_stage_hardshadow bad = shadow( 5 ); bad.pos.y = inf; EXPECT( refused( bad, "finite" ) ); }
        { acn_stage_hardshadow bad = shadow( 5 ); bad.d.x = nan; EXPECT( refused( bad, "finite" ) ); }
        /* one workgroup per 256 records, 64 at most */
        {
            std::vector< acn_stage_hardshadow > q( 257, shadow( 0 ) );
            acn_stage_args b = a; b.n = 257; b.in = q.data();
            EXPECT( acn_stage_check( true, &b, sc, &caps, &msg ) == ACN_OK && caps.grid == 2 && caps.cap_hard_shadow == 257 );
            q.assign( 64 * 256 + 1, shadow( ACN_STAGE_DEAD ) );
            b.n = ( uint32_t )q.size(); b.in = q.data();
            EXPECT( acn_stage_check( true, &b, sc, &caps, &msg ) == ACN_OK && caps.grid == 64 );
        }
    }

    /* ---- k_hard_path ---- */
    {
        std::vector< acn_stage_hardpath > r;
        for( uint32_t i = 0; i < 5; i++ ) r.push_back( path( i ) );
        r[ 1 ].resume = 0;                                /* every element is to be folded */
        r[ 2 ] = path( ACN_STAGE_DEAD, 1u, -9 );          /* dead: not read further */
        r[ 2 ].d.z = inf;
        r[ 4 ].depth = ACN_STAGE_MAX_DEPTH;
        acn_stage_args a;
        memset( &a, 0, sizeof( a ) );
        a.stage = ACN_STAGE_HARD_PATH; a.n = 5; a.in = r.data();
        EXPECT( acn_stage_check( true, &a, sc, &caps, &msg ) == ACN_OK );
        /* a hit record per ray at most, and one reservation per wave */
        EXPECT( caps.grid == 1 && caps.chunk == 64 && caps.cap_hard_path == 5 && caps.cap_children == 5 + 1 * 4 * 64 );
        EXPECT( caps.cap_tasks == 0 && caps.cap_rays == 0 && caps.cap_hard_shadow == 0 );
        { acn_stage_args b = a; b.cls = 3; EXPECT( acn_stage_check( true, &b, sc, &caps, &msg ) == ACN_OK && caps.grid == 3 && caps.cap_children == 5 + 3 * 4 * 64 ); }
        { acn_stage_args b = a; b.cls = 1000; EXPECT( acn_stage_check( true, &b, sc, &caps, &msg ) == ACN_ERR_ARG && says( msg, "workgroups" ) ); }
        auto refused = [ & ]( acn_stage_hardpath bad, const char* word )
        {
            std::vector< acn_stage_hardpath > q = r;
            q[ 4 ] = bad;
            acn_stage_args b = a; b.in = q.data();
            msg.clear();
            return acn_stage_check( true, &b, sc, &caps, &msg ) == ACN_ERR_ARG && says( msg, word ) && says( msg, "hard-path record 4" );
        };
        EXPECT( refused( path( 5 ), "pixel" ) );
        EXPECT( refused( path( 4, 6u, -1 ), "depth" ) );
        EXPECT( refused( path( 4, 6u, ACN_STAGE_MAX_DEPTH + 1 ), "depth" ) );
        EXPECT( refused( path( 4, 7u ), "bit 0" ) );
        EXPECT( refused( path( 4, 1u ), "bit 0" ) );
        EXPECT( refused( path( 4, 8u ), "resume flag" ) );
        { acn_stage_hardpath bad = path( 4 ); bad.pos.z = -inf; EXPECT( refused( bad, "finite" ) ); }
        { acn_stage_hardpath bad = path( 4 ); bad.d.y = nan; EXPECT( refused( bad, "finite" ) ); }
        EXPECT( !refused( path( 4, 2u, 0 ), "depth" ) && msg.empty() );
    }

    if( failures ) { printf( "%d checks failed\n", failures ); return 1; }
    printf( "ok\n" );
    return 0;
}
