/* tables_cpu.cpp -- test shim: the upload's scene tables (actinon_amd/csrc/acn_tables.cpp) built on the CPU and copied out
 * table by table (tests/test_tables_cpu.py). */
#include <string.h>
#include "acn_tables.h"

enum { T_NODES = 0, T_MATS, T_ELEMS, T_SC_TABLE, T_SC_SPHERES };

/* switches: no_leaf_pairs, no_pair2, no_prune_levels, no_simple_compounds, no_sc_cull, no_sc_reversed; prune_min / lds_max < 0: not given */
extern "C" void* tables_build( const acn_flat_scene* scene, const int* switches, long long prune_min, long long lds_max )
{
    acn_table_opts o;
    o.no_leaf_pairs = switches[ 0 ]; o.no_pair2 = switches[ 1 ]; o.no_prune_levels = switches[ 2 ];
    o.no_simple_compounds = switches[ 3 ]; o.no_sc_cull = switches[ 4 ]; o.no_sc_reversed = switches[ 5 ];
    if( prune_min >= 0 ) o.prune_min = ( size_t )prune_min;
    if( lds_max >= 0 ) { o.lds_max = ( size_t )lds_max; o.lds_max_set = true; }
    acn_scene_tables* t = new acn_scene_tables();
    acn_tables_build( scene, o, t );
    return t;
}

static const void* table( const acn_scene_tables* t, int which, size_t* bytes )
{
    switch( which )
    {
        case T_NODES:      *bytes = sizeof( GNode ) * t->nodes.size();        return t->nodes.data();
        case T_MATS:       *bytes = sizeof( GMat ) * t->mats.size();          return t->mats.data();
        case T_ELEMS:      *bytes = sizeof( int32_t ) * t->elems.size();      return t->elems.data();
        case T_SC_TABLE:   *bytes = sizeof( SCEntry ) * t->sc_table.size();   return t->sc_table.data();
        case T_SC_SPHERES: *bytes = sizeof( double ) * t->sc_spheres.size();  return t->sc_spheres.data();
        default:           *bytes = 0;                                        return nullptr;
    }
}
extern "C" size_t tables_bytes( const void* t, int which ) { size_t n = 0; table( ( const acn_scene_tables* )t, which, &n ); return n; }
extern "C" void tables_copy( const void* t, int which, void* dst ) { size_t n = 0; const void* p = table( ( const acn_scene_tables* )t, which, &n ); if( n ) memcpy( dst, p, n ); }
/* prune_base, elem_pos_base, prune, leaf_lights, n_lights, n_levels, lds_bytes, lds_stack_bytes */
extern "C" void tables_scalars( const void* tp, unsigned long long* out )
{
    const acn_scene_tables* t = ( const acn_scene_tables* )tp;
    out[ 0 ] = t->prune_base; out[ 1 ] = t->elem_pos_base; out[ 2 ] = t->prune; out[ 3 ] = t->leaf_lights;
    out[ 4 ] = t->n_lights; out[ 5 ] = ( unsigned long long )t->n_levels; out[ 6 ] = t->lds_bytes; out[ 7 ] = t->lds_stack_bytes;
}
extern "C" void tables_free( void* t ) { delete ( acn_scene_tables* )t; }

extern "C" int tables_validate( const acn_flat_scene* scene, int* max_csg, char* err, size_t cap )
{
    std::string e;
    int st = acn_tables_validate( scene, max_csg, &e );
    if( cap ) { strncpy( err, e.c_str(), cap - 1 ); err[ cap - 1 ] = 0; }
    return st;
}
