/* actinon_amd/csrc/acn_stage_host.h on its own, the walk (acn_stage_walk_check: what acn_stage_walk_plan / acn_run_stage_walk do
 * before anything is launched): a program that tests/test_stage_walk_cpu.py builds with -fsanitize=address,undefined and runs.  Every
 * refusal and the plan of an accepted call, with the rays in heap blocks of exactly their size, so a read past ray n - 1 -- or any
 * read of the rays in the camera form -- is a sanitizer report.  The program prints "ok" and returns 0, or names what failed. */
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "acn_stage_host.h"

static int failures = 0;
#define EXPECT( cond ) do { if( !( cond ) ) { printf( "line %d: %s\n", __LINE__, #cond ); failures++; } } while( 0 )
static bool says( const std::string& msg, const char* word ) { return msg.find( word ) != std::string::npos; }

static const double TMIN = 0.002;

static acn_stage_raytask ray( uint32_t pixel, int depth = 22, double intensity = 1.0 )
{
    acn_stage_raytask r;
    memset( &r, 0, sizeof( r ) );
    r.d.z = 1; r.T.x = r.T.y = r.T.z = 0.5; r.intensity = intensity; r.depth = depth; r.pixel = pixel;
    return r;
}

int main()
{
    static_assert( sizeof( acn_stage_raytask ) == 88, "record sizes: DESIGN.md section 3" );
    static_assert( sizeof( acn_stage_walk_args ) == 72, "acn_stage_walk_args: actinon_amd/abi.py restates it" );
    acn_stage_scene sc = { 7u, 2u, 50u, 16u, TMIN };
    std::string msg;
    acn_stage_caps caps;
    const double inf = std::numeric_limits< double >::infinity(), nan = std::nan( "" );

    std::vector< acn_stage_raytask > r;
    for( uint32_t i = 0; i < 6; i++ ) r.push_back( ray( i ) );
    r[ 1 ].depth = 1;                                     /* every child a probe */
    r[ 2 ].intensity = TMIN;                              /* the least a queued ray carries */
    r[ 3 ] = ray( ACN_STAGE_DEAD, -9, nan );              /* a dead slot is not read further */
    r[ 3 ].p.x = nan; r[ 3 ].d.z = 0; r[ 3 ].T.y = inf;
    r[ 4 ].depth = ACN_STAGE_MAX_DEPTH;
    r[ 5 ].T.x = 0; r[ 5 ].T.y = -2.0;                    /* any finite throughput */
    acn_stage_walk_args a;
    memset( &a, 0, sizeof( a ) );
    a.stage = ACN_STAGE_WALK; a.n = 6; a.in = r.data(); a.passes = 1; a.private_limit = 0xFFFFFFFFu; a.stack_cap = 512; a.fetch = 64; a.room_rays = 100;

    /* ---- an accepted call and its plan: one workgroup, a reservation of 64 per wave, queue and launch ---- */
    EXPECT( acn_stage_walk_check( true, &a, sc, &caps, &msg ) == ACN_OK );
    EXPECT( caps.grid == 1 && caps.chunk == 64 && caps.cap_rays == 100 + 256 && caps.cap_tasks == 100 + 256 && caps.cap_hard_shadow == 300 + 256 );
    EXPECT( caps.cap_children == 0 && caps.cap_hard_path == 0 );
    { acn_stage_walk_args b = a; b.passes = 32; b.grid = 3; EXPECT( acn_stage_walk_check( true, &b, sc, &caps, &msg ) == ACN_OK );
      EXPECT( caps.grid == 3 && caps.cap_rays == 100 + 768 && caps.cap_tasks == 100 + 32 * 768 && caps.cap_hard_shadow == 300 + 32 * 768 ); }
    { acn_stage_walk_args b = a; b.grid = 64; b.stack_cap = ACN_STAGE_WALK_MAX_STACK; b.stack_use = b.stack_cap; b.fetch = ACN_STAGE_MAX_RECORDS; b.private_limit = 0;
      b.flags = ACN_STAGE_NO_PRUNE | ACN_STAGE_NO_EMIT_TERMS | ACN_STAGE_GLOBAL_NODES | ACN_STAGE_COUNT_WORK;
      EXPECT( acn_stage_walk_check( true, &b, sc, &caps, &msg ) == ACN_OK && caps.grid == 64 ); }
    { acn_stage_walk_args b = a; b.stack_cap = 1; b.stack_use = 1; EXPECT( acn_stage_walk_check( true, &b, sc, &caps, &msg ) == ACN_OK ); }
    { acn_stage_walk_args b = a; b.room_rays = 6; EXPECT( acn_stage_walk_check( true, &b, sc, &caps, &msg ) == ACN_OK && caps.cap_rays == 6 + 256 ); }
    /* the grid by n: one workgroup per 256 slots, 64 at most */
    {
        std::vector< acn_stage_raytask > q( 257, ray( 0 ) );
        acn_stage_walk_args b = a; b.n = 257; b.in = q.data(); b.room_rays = 257;
        EXPECT( acn_stage_walk_check( true, &b, sc, &caps, &msg ) == ACN_OK && caps.grid == 2 );
        q.assign( 64 * 256 + 1, ray( ACN_STAGE_DEAD ) );
        b.n = ( uint32_t )q.size(); b.in = q.data(); b.room_rays = b.n;
        EXPECT( acn_stage_walk_check( true, &b, sc, &caps, &msg ) == ACN_OK && caps.grid == 64 );
    }
    /* the camera form reads no ray: positions, or the raster; the launch covers the slots of whole tiles */
    {
        std::vector< double > pos( 2 * 300, 1.5 );
        acn_stage_walk_args b = a; b.in = nullptr; b.camera = 1; b.n = 300; b.room_rays = 300; b.pos_xy = pos.data();
        EXPECT( acn_stage_walk_check( true, &b, sc, &caps, &msg ) == ACN_OK && caps.grid == 2 && acn_stage_walk_slots( &b ) == 512 );
        b.pos_xy = nullptr; b.first_pixel = 17;
        EXPECT( acn_stage_walk_check( true, &b, sc, &caps, &msg ) == ACN_OK && caps.grid == 2 );
        b.n = 256; b.room_rays = 256;
        EXPECT( acn_stage_walk_check( true, &b, sc, &caps, &msg ) == ACN_OK && caps.grid == 1 && acn_stage_walk_slots( &b ) == 256 );
        b.in = r.data();
        EXPECT( acn_stage_walk_check( true, &b, sc, &caps, &msg ) == ACN_ERR_ARG && says( msg, "both input forms" ) );
    }

    /* ---- refusals of the arguments ---- */
    EXPECT( acn_stage_walk_check( false, &a, sc, &caps, &msg ) == ACN_ERR_ARG && says( msg, "handle" ) );
    EXPECT( acn_stage_walk_check( true, nullptr, sc, &caps, &msg ) == ACN_ERR_ARG && says( msg, "null argument" ) );
    EXPECT( acn_stage_walk_check( true, &a, sc, nullptr, &msg ) == ACN_ERR_ARG && says( msg, "null argument" ) );
    auto refused_args = [ & ]( acn_stage_walk_args b, const char* word )
    {
        msg.clear();
        return acn_stage_walk_check( true, &b, sc, &caps, &msg ) == ACN_ERR_ARG && says( msg, word );
    };
    { acn_stage_walk_args b = a; b.stage = ACN_STAGE_SHADE_HITS; EXPECT( refused_args( b, "ACN_STAGE_WALK" ) ); }
    { acn_stage_walk_args b = a; b.flags = ACN_STAGE_NO_LEAF_LIGHTS; EXPECT( refused_args( b, "flags" ) ); }
    { acn_stage_walk_args b = a; b.flags = ACN_STAGE_COUNT_WORK; EXPECT( acn_stage_walk_check( true, &b, sc, &caps, &msg ) == ACN_OK ); }   /* bit 16: the counting variants */
    { acn_stage_walk_args b = a; b.flags = 32; EXPECT( refused_args( b, "flags" ) ); }
    { acn_stage_walk_args b = a; b.flags = ACN_STAGE_COUNT_WORK | ACN_STAGE_NO_LEAF_LIGHTS; EXPECT( refused_args( b, "flags" ) ); }
    { acn_stage_walk_args b = a; b.in = nullptr; EXPECT( refused_args( b, "neither input form" ) ); }
    { std::vector< double > pos( 12, 0.5 ); acn_stage_walk_args b = a; b.pos_xy = pos.data(); EXPECT( refused_args( b, "both input forms" ) ); }
    { acn_stage_walk_args b = a; b.n = 0; EXPECT( refused_args( b, "records" ) ); }
    { acn_stage_walk_args b = a; b.in = nullptr; b.camera = 1; b.n = ACN_STAGE_MAX_RECORDS + 1; b.room_rays = b.n; EXPECT( refused_args( b, "records" ) ); }
    { acn_stage_walk_args b = a; b.passes = 0; EXPECT( refused_args( b, "passes" ) ); }
    { acn_stage_walk_args b = a; b.passes = ACN_MAX_WALK_PASSES + 1; EXPECT( refused_args( b, "passes" ) ); }
    { acn_stage_walk_args b = a; b.stack_cap = 0; EXPECT( refused_args( b, "stack_cap" ) ); }
    { acn_stage_walk_args b = a; b.stack_cap = ACN_STAGE_WALK_MAX_STACK + 1; EXPECT( refused_args( b, "stack_cap" ) ); }
    { acn_stage_walk_args b = a; b.stack_use = 513; EXPECT( refused_args( b, "stack_use" ) ); }
    { acn_stage_walk_args b = a; b.fetch = 63; EXPECT( refused_args( b, "fetch" ) ); }
    { acn_stage_walk_args b = a; b.fetch = 0; EXPECT( refused_args( b, "fetch" ) ); }
    { acn_stage_walk_args b = a; b.fetch = ACN_STAGE_MAX_RECORDS + 1; EXPECT( refused_args( b, "fetch" ) ); }
    { acn_stage_walk_args b = a; b.grid = 65; EXPECT( refused_args( b, "workgroups" ) ); }
    { acn_stage_walk_args b = a; b.room_rays = 5; EXPECT( refused_args( b, "room_rays" ) ); }
    { acn_stage_walk_args b = a; b.room_rays = 0; EXPECT( refused_args( b, "room_rays" ) ); }
    { acn_stage_walk_args b = a; b.room_rays = ACN_STAGE_MAX_CAP / 3; EXPECT( refused_args( b, "above 2^26" ) ); }
    { acn_stage_walk_args b = a; b.room_rays = 0xFFFFFFFFu; EXPECT( refused_args( b, "above 2^26" ) ); }

    /* ---- refusals of a ray: the last record, so that the loop reaches the end of the block ---- */
    auto refused = [ & ]( acn_stage_raytask bad, const char* word )
    {
        std::vector< acn_stage_raytask > q = r;
        q[ 5 ] = bad;
        acn_stage_walk_args b = a; b.in = q.data();
        msg.clear();
        return acn_stage_walk_check( true, &b, sc, &caps, &msg ) == ACN_ERR_ARG && says( msg, word ) && says( msg, "ray 5" );
    };
    EXPECT( refused( ray( 6 ), "pixel" ) );
    EXPECT( refused( ray( 0xFFFFFFFEu ), "pixel" ) );
    { acn_stage_raytask bad = ray( 5 ); bad.p.y = inf; EXPECT( refused( bad, "not finite" ) ); }
    { acn_stage_raytask bad = ray( 5 ); bad.d.x = nan; EXPECT( refused( bad, "not finite" ) ); }
    { acn_stage_raytask bad = ray( 5 ); bad.T.z = nan; EXPECT( refused( bad, "T is not finite" ) ); }
    { acn_stage_raytask bad = ray( 5 ); bad.T.x = -inf; EXPECT( refused( bad, "T is not finite" ) ); }
    { acn_stage_raytask bad = ray( 5 ); bad.d.z = 0; EXPECT( refused( bad, "no length" ) ); }
    { acn_stage_raytask bad = ray( 5 ); bad.d.z = -0.0; EXPECT( refused( bad, "no length" ) ); }
    EXPECT( refused( ray( 5, 0 ), "depth" ) );
    EXPECT( refused( ray( 5, -1 ), "depth" ) );
    EXPECT( refused( ray( 5, ACN_STAGE_MAX_DEPTH + 1 ), "depth" ) );
    EXPECT( refused( ray( 5, 22, nan ), "intensity" ) );
    EXPECT( refused( ray( 5, 22, inf ), "intensity" ) );
    EXPECT( refused( ray( 5, 22, -1.0 ), "intensity" ) );
    EXPECT( refused( ray( 5, 22, 0.0 ), "intensity" ) );
    EXPECT( refused( ray( 5, 22, std::nextafter( TMIN, 0.0 ) ), "intensity" ) );
    EXPECT( !refused( ray( 5, 22, TMIN ), "intensity" ) && msg.empty() );
    EXPECT( !refused( ray( 5, 1, std::nextafter( TMIN, 1.0 ) ), "intensity" ) && msg.empty() );
    /* a scene that traces every ray, however faint */
    sc.trace_min_intensity = 0.0;
    EXPECT( !refused( ray( 5, 22, 0.0 ), "intensity" ) && msg.empty() );
    EXPECT( refused( ray( 5, 22, -1e-300 ), "intensity" ) );

    if( failures ) { printf( "%d checks failed\n", failures ); return 1; }
    printf( "ok\n" );
    return 0;
}
