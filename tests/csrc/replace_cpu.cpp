/* The host-only rules of a change of scene on a live handle (acn_scene_replace, acn_scene_set_params), twice.  As a shared library
 * it is the extern "C" shim through which tests/test_replace_cpu.py compares acn_replace_keeps_learned (actinon_amd/csrc/acn_queueplan.h)
 * with a Python model, and acn_tables_validate_params / acn_tables_levels (actinon_amd/csrc/acn_tables.cpp, compiled beside this file)
 * with what the whole-scene path -- acn_tables_validate, acn_tables_build -- says about a small scene with the same parameters.  With
 * -DREPLACE_CPU_MAIN it is a program that the same test builds with -fsanitize=address,undefined and runs: every object in a heap
 * block of exactly its size.  The program prints "ok" and returns 0, or names what failed. */
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>

#include "acn_queueplan.h"
#include "acn_tables.h"

/* a light root with one radiant sphere, a matter root with one sphere: the least acn_tables_validate accepts */
struct SmallScene
{
    std::unique_ptr< acn_node[] > nodes{ new acn_node[ 4 ] };
    std::unique_ptr< int32_t[] > elems{ new int32_t[ 2 ] };
    acn_flat_scene flat;
    explicit SmallScene( const acn_params& prm )
    {
        memset( nodes.get(), 0, sizeof( acn_node ) * 4 );
        for( int i = 0; i < 4; i++ )
        {
            acn_node& n = nodes[ i ];
            n.type = i < 2 ? ACN_COMPOUND : ACN_SPHERE; n.child0 = n.child1 = -1; n.texture = -1;
            n.rax[ 0 ] = n.rax[ 4 ] = n.rax[ 8 ] = 1.0; n.prm[ 0 ] = 1.0; n.refractive_index = 1.0; n.diffuse_reflectivity = 1.0;
            n.color[ 0 ] = n.color[ 1 ] = n.color[ 2 ] = 0.5;
        }
        nodes[ 0 ].child0 = 0; nodes[ 0 ].child1 = 1;   /* light: elems[ 0 ] */
        nodes[ 1 ].child0 = 1; nodes[ 1 ].child1 = 1;   /* matter: elems[ 1 ] */
        nodes[ 2 ].radiance = 5.0; nodes[ 2 ].pos[ 2 ] = 10.0;
        elems[ 0 ] = 2; elems[ 1 ] = 3;
        memset( &flat, 0, sizeof( flat ) );
        flat.abi_version = ACN_ABI_VERSION; flat.n_nodes = 4; flat.n_elems = 2; flat.light_root = 0; flat.matter_root = 1;
        flat.nodes = nodes.get(); flat.elems = elems.get(); flat.params = prm;
    }
};

extern "C" {

size_t rc_kind_size( void ) { return sizeof( acn_scene_kind ); }
int rc_keeps_learned( const acn_scene_kind* was, const acn_scene_kind* now ) { return acn_replace_keeps_learned( was, now ); }

int rc_validate_params( const acn_params* prm ) { std::string err; return acn_tables_validate_params( prm, &err ); }
int rc_levels( const acn_params* prm ) { return acn_tables_levels( prm ); }
/* the whole-scene path on a small scene with these parameters: the status of acn_tables_validate, and where it is ACN_OK the path
 * levels acn_tables_build plans */
int rc_scene_status( const acn_params* prm, int* n_levels )
{
    SmallScene s( *prm );
    int max_csg = 0; std::string err;
    const int st = acn_tables_validate( &s.flat, &max_csg, &err );
    if( st == ACN_OK && n_levels )
    {
        acn_scene_tables t;
        acn_tables_build( &s.flat, acn_table_opts(), &t );
        *n_levels = t.n_levels;
    }
    return st;
}

}

#ifdef REPLACE_CPU_MAIN
#define CHECK( cond ) do { if( !( cond ) ) { printf( "failed: %s (line %d)\n", #cond, __LINE__ ); return 1; } } while( 0 )

static acn_params good_params()
{
    acn_params p;
    memset( &p, 0, sizeof( p ) );
    p.image_width = 64; p.image_height = 36; p.gamma = 1.0;
    p.camera_position[ 1 ] = -20.0; p.camera_view_direction[ 1 ] = 1.0; p.camera_top_direction[ 2 ] = 1.0; p.camera_focal_length = 2.0;
    p.trace_depth = 11; p.trace_min_intensity = 0.01; p.direct_samples = 50; p.path_samples = 16; p.max_path_length = 1e30;
    return p;
}

int main()
{
    /* the kind rule: each member alone, and the double by its bits */
    std::unique_ptr< acn_scene_kind > a( new acn_scene_kind ), b( new acn_scene_kind );
    memset( a.get(), 0, sizeof( acn_scene_kind ) );
    a->n_nodes = 18; a->n_elems = 12; a->n_lights = 2; a->n_levels = 2; a->prune = 1; a->path_samples = 64; a->direct_samples = 50;
    a->trace_depth = 11; a->trace_min_intensity = 0.01;
    *b = *a;
    CHECK( acn_replace_keeps_learned( a.get(), b.get() ) == 1 );
    for( int m = 0; m < 9; m++ )
    {
        *b = *a;
        switch( m )
        {
            case 0: b->n_nodes++; break;         case 1: b->n_elems++; break;          case 2: b->n_lights++; break;
            case 3: b->n_levels++; break;        case 4: b->prune = 0; break;          case 5: b->path_samples = 16; break;
            case 6: b->direct_samples++; break;  case 7: b->trace_depth = 21; break;
            default: { uint64_t bits; memcpy( &bits, &b->trace_min_intensity, 8 ); bits ^= 1; memcpy( &b->trace_min_intensity, &bits, 8 ); }
        }
        CHECK( acn_replace_keeps_learned( a.get(), b.get() ) == 0 );
        CHECK( acn_replace_keeps_learned( b.get(), a.get() ) == 0 );
    }
    *b = *a; a->trace_min_intensity = 0.0; b->trace_min_intensity = -0.0;
    CHECK( acn_replace_keeps_learned( a.get(), b.get() ) == 0 );
    b->trace_min_intensity = 0.0;
    CHECK( acn_replace_keeps_learned( a.get(), b.get() ) == 1 );

    /* the parameter checks and the path levels against the whole-scene path */
    std::unique_ptr< acn_params > p( new acn_params( good_params() ) );
    int levels = 0;
    CHECK( rc_validate_params( p.get() ) == ACN_OK && rc_scene_status( p.get(), &levels ) == ACN_OK && levels == rc_levels( p.get() ) && levels == 2 );
    const uint64_t depths[] = { 0, 1, 10, 11, 20, 21, 30, 31, 59, 60, 61 };
    for( uint64_t samples : { 0ull, 1ull, 64ull } )
        for( uint64_t d : depths )
        {
            *p = good_params(); p->trace_depth = d; p->path_samples = samples;
            levels = -1;
            const int st = rc_scene_status( p.get(), &levels );
            CHECK( st == rc_validate_params( p.get() ) );
            CHECK( st == ( d > 10 * ACN_MAX_PATH_LEVELS + 10 ? ACN_ERR_UNSUPPORTED : ACN_OK ) );
            if( st == ACN_OK ) CHECK( levels == rc_levels( p.get() ) && levels >= 1 && levels <= ACN_MAX_PATH_LEVELS + 1 );
        }
    *p = good_params(); p->experimental_level = 1;
    CHECK( rc_validate_params( p.get() ) == ACN_ERR_UNSUPPORTED && rc_scene_status( p.get(), nullptr ) == ACN_ERR_UNSUPPORTED );
    *p = good_params(); p->image_height = 1;
    CHECK( rc_validate_params( p.get() ) == ACN_ERR_ARG && rc_scene_status( p.get(), nullptr ) == ACN_ERR_ARG );
    *p = good_params(); p->image_width = 0;
    CHECK( rc_validate_params( p.get() ) == ACN_ERR_ARG && rc_scene_status( p.get(), nullptr ) == ACN_ERR_ARG );
    *p = good_params(); p->image_height = 2; p->image_width = 1;
    CHECK( rc_validate_params( p.get() ) == ACN_OK && rc_scene_status( p.get(), nullptr ) == ACN_OK );
    printf( "ok\n" );
    return 0;
}
#endif
