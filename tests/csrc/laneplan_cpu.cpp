/* acn_lane_plan of actinon_amd/csrc/acn_queueplan.h on its own, twice.  As a shared library it is the extern "C" shim through
 * which tests/test_laneplan_cpu.py compares the plan with a Python model.  With -DLANEPLAN_CPU_MAIN it is a program that the same
 * test builds with -fsanitize=address,undefined and runs: the plan at the edges of its arguments, the results written into a
 * heap block of exactly their size.  The program prints "ok" and returns 0, or names what failed. */
#include <climits>
#include <cstdio>
#include <memory>

#include "acn_queueplan.h"

extern "C"
{
/* out[ 4 ]: lanes, grid, shade_grid, walk_grid */
void lp_lane_plan( int lanes_given, int lanes_env, unsigned cus, unsigned grid_env, unsigned shade_grid_env, unsigned walk_grid_env, uint32_t* out )
{
    const acn_lane_plan_t p = acn_lane_plan( lanes_given, lanes_env, cus, grid_env, shade_grid_env, walk_grid_env );
    out[ 0 ] = ( uint32_t )p.lanes; out[ 1 ] = p.grid; out[ 2 ] = p.shade_grid; out[ 3 ] = p.walk_grid;
}
int lp_default_lanes( void ) { return ACN_DEFAULT_LANES; }
int lp_default_lane_wgs( void ) { return ACN_DEFAULT_LANE_WGS; }
int lp_max_lanes( void ) { return ACN_MAX_LANES; }
int lp_lanes_for_counts( int tun_lanes, uint64_t n, uint64_t ps ) { return acn_lanes_for_counts( tun_lanes, ( size_t )n, ps ); }
}

#ifdef LANEPLAN_CPU_MAIN
static int failures = 0;
#define EXPECT( cond ) do { if( !( cond ) ) { printf( "line %d: %s\n", __LINE__, #cond ); failures++; } } while( 0 )

int main()
{
    std::unique_ptr< uint32_t[] > out( new uint32_t[ 4 ] );
    /* the default: no ACN_LANES, whatever value the unread variable is said to have */
    for( int env : { INT_MIN, -1, 0, 1, 6, INT_MAX } )
    {
        lp_lane_plan( 0, env, 256, 0, 0, 0, out.get() );
        EXPECT( out[ 0 ] == ACN_DEFAULT_LANES && out[ 1 ] == 256u * ACN_DEFAULT_LANE_WGS && out[ 2 ] == 256u * ACN_DEFAULT_LANE_WGS && out[ 3 ] == out[ 1 ] );
    }
    /* a given count: clamped to 1 .. ACN_MAX_LANES, on one workgroup per compute unit (k_shade one and a half) */
    lp_lane_plan( 1, 6, 256, 0, 0, 0, out.get() );
    EXPECT( out[ 0 ] == 6 && out[ 1 ] == 256 && out[ 2 ] == 384 && out[ 3 ] == 256 );
    lp_lane_plan( 1, INT_MIN, 1, 0, 0, 0, out.get() );
    EXPECT( out[ 0 ] == 1 && out[ 1 ] == 1 && out[ 2 ] == 1 && out[ 3 ] == 1 );
    lp_lane_plan( 1, INT_MAX, 304, 0, 0, 0, out.get() );
    EXPECT( out[ 0 ] == ACN_MAX_LANES && out[ 1 ] == 304 && out[ 2 ] == 456 && out[ 3 ] == 304 );
    /* the grids of the environment override, each for itself; k_walk follows ACN_GRID */
    lp_lane_plan( 0, 0, 256, 100, 0, 0, out.get() );
    EXPECT( out[ 1 ] == 100 && out[ 2 ] == 256u * ACN_DEFAULT_LANE_WGS && out[ 3 ] == 100 );
    lp_lane_plan( 1, 4, 256, 0, UINT_MAX, 7, out.get() );
    EXPECT( out[ 0 ] == 4 && out[ 1 ] == 256 && out[ 2 ] == UINT_MAX && out[ 3 ] == 7 );
    /* unsigned arithmetic wraps, it does not trap: a device of 2^31 compute units is not one, but no argument is undefined */
    lp_lane_plan( 1, 2, 0x80000000u, 0, 0, 0, out.get() );
    EXPECT( out[ 1 ] == 0x80000000u && out[ 2 ] == ( 0x80000000u * 3u ) / 2u );
    lp_lane_plan( 0, 0, 0, 0, 0, 0, out.get() );
    EXPECT( out[ 0 ] == ACN_DEFAULT_LANES && out[ 1 ] == 0 && out[ 2 ] == 0 && out[ 3 ] == 0 );
    if( failures == 0 ) printf( "ok\n" );
    return failures ? 1 : 0;
}
#endif
