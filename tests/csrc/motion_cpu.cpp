/* actinon_amd/csrc/acn_motion_host.h on its own: a program that tests/test_motion_cpu.py builds with -fsanitize=address,undefined and
 * runs.  The checks of the motion table of acn_reproject_moving*, and acn_motion_from_scenes on small hand-made scenes whose arrays are
 * heap blocks of exactly their size, so a read or write past one is a sanitizer report: identical scenes, a moved node, a changed
 * one, a skewed one, another shape, a scale node with an equal and with an unequal subtree, textures, and every refusal.  The program
 * prints "ok" and returns 0, or names what failed. */
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "acn_motion_host.h"

static int failures = 0;
#define EXPECT( cond ) do { if( !( cond ) ) { printf( "line %d: %s\n", __LINE__, #cond ); failures++; } } while( 0 )

static bool says( const std::string& msg, const char* word ) { return msg.find( word ) != std::string::npos; }

/* a scene that owns its arrays: vectors sized exactly */
struct Scene
{
    std::vector< acn_node > nodes;
    std::vector< int32_t > elems;
    std::vector< acn_texture > textures;
    acn_flat_scene flat;
    const acn_flat_scene* c()
    {
        flat = acn_flat_scene{};
        flat.abi_version = ACN_ABI_VERSION;
        flat.n_nodes = ( uint32_t )nodes.size(); flat.n_elems = ( uint32_t )elems.size(); flat.n_textures = ( uint32_t )textures.size();
        flat.light_root = 0; flat.matter_root = 1;
        flat.nodes = nodes.data(); flat.elems = elems.data(); flat.textures = textures.data();
        return &flat;
    }
};

static acn_node node_of( int32_t type, int32_t child0 = -1, int32_t child1 = -1 )
{
    acn_node n;
    memset( &n, 0, sizeof( n ) );
    n.type = type; n.child0 = child0; n.child1 = child1; n.texture = -1;
    n.rax[ 0 ] = n.rax[ 4 ] = n.rax[ 8 ] = 1.0;
    n.color[ 0 ] = n.color[ 1 ] = n.color[ 2 ] = 0.5;
    n.diffuse_reflectivity = 1.0;
    return n;
}

/* 0: light compound (no elements), 1: matter compound of 2, 3 and 4; 2: a sphere with texture 0; 3: a scale node over 5; 4: a pair of 6 and 7 */
static Scene base_scene()
{
    Scene s;
    s.nodes.push_back( node_of( ACN_COMPOUND, 0, 0 ) );
    s.nodes.push_back( node_of( ACN_COMPOUND, 0, 3 ) );
    s.nodes.push_back( node_of( ACN_SPHERE ) );
    s.nodes.push_back( node_of( ACN_SCALE, 5 ) );
    s.nodes.push_back( node_of( ACN_PAIR_INSIDE, 6, 7 ) );
    s.nodes.push_back( node_of( ACN_SPHERE ) );
    s.nodes.push_back( node_of( ACN_SPHERE ) );
    s.nodes.push_back( node_of( ACN_SQUAROID ) );
    s.elems = { 2, 3, 4 };
    s.nodes[ 2 ].prm[ 0 ] = 0.9; s.nodes[ 2 ].texture = 0;
    s.nodes[ 2 ].pos[ 0 ] = -1.2;
    s.nodes[ 3 ].prm[ 0 ] = 1.0; s.nodes[ 3 ].prm[ 1 ] = 1.0; s.nodes[ 3 ].prm[ 2 ] = 2.0;
    s.nodes[ 5 ].prm[ 0 ] = 0.3;
    acn_texture t;
    memset( &t, 0, sizeof( t ) );
    t.kind = ACN_TXM_CHESS; t.color1[ 0 ] = 0.9; t.color2[ 1 ] = 0.9; t.scale = 4.0;
    s.textures.push_back( t );
    return s;
}

/* node i turned a quarter about z and moved to pos */
static void quarter_turn( acn_node& n, double x, double y, double z )
{
    const double r[ 9 ] = { 0.0, -1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0 };
    memcpy( n.rax, r, sizeof( r ) );
    n.pos[ 0 ] = x; n.pos[ 1 ] = y; n.pos[ 2 ] = z;
}

struct Result { int status; std::vector< double > table; acn_motion_report rep; std::string msg; };

static Result run( Scene& prev, Scene& cur, double cap = 0.0 )
{
    Result r;
    r.table.assign( cur.nodes.size() * ACN_MOTION_STRIDE, 7.25 );
    r.rep = acn_motion_report{ 9u, 9u, 9u, 9u };
    r.status = acn_motion_from_scenes_impl( prev.c(), cur.c(), cap, r.table.data(), &r.rep, &r.msg );
    return r;
}

static double state( const Result& r, size_t i ) { return r.table[ i * ACN_MOTION_STRIDE + 12 ]; }

int main()
{
    std::string msg;
    const double inf = std::numeric_limits< double >::infinity(), nan = std::nan( "" );

    /* the table of a call */
    alignas( 16 ) static double buf[ 64 ];
    EXPECT( acn_motion_table_check( buf, 4, 10, &msg ) == ACN_OK );
    EXPECT( acn_motion_table_check( nullptr, 0, 0, &msg ) == ACN_OK );                                              /* nothing to do */
    EXPECT( acn_motion_table_check( nullptr, 4, 10, &msg ) == ACN_ERR_ARG && says( msg, "null" ) && says( msg, "motion" ) );
    EXPECT( acn_motion_table_check( buf, 0, 10, &msg ) == ACN_ERR_ARG && says( msg, "n_motion" ) );
    EXPECT( acn_motion_table_check( ( const char* )buf + 8, 4, 10, &msg ) == ACN_ERR_ARG && says( msg, "align" ) );
    EXPECT( acn_motion_table_check( buf, ( uint64_t )1 << 31, 10, &msg ) == ACN_OK );
    EXPECT( acn_motion_table_check( buf, ( ( uint64_t )1 << 31 ) + 1, 10, &msg ) == ACN_ERR_ARG && says( msg, "2^31" ) );

    /* identical scenes: all REST, rows of zeros */
    {
        Scene a = base_scene(), b = base_scene();
        Result r = run( a, b );
        EXPECT( r.status == ACN_OK && r.rep.same_shape == 1 && r.rep.n_rest == 8 && r.rep.n_moved == 0 && r.rep.n_none == 0 );
        for( double v : r.table ) EXPECT( v == 0.0 );
    }
    /* the sphere turned and moved: A = rax_prev^T * rax_cur, t = pos_prev - A * pos_cur; the cap */
    {
        Scene a = base_scene(), b = base_scene();
        quarter_turn( b.nodes[ 2 ], 2.0, 3.0, 4.0 );
        Result r = run( a, b, 8.0 );
        const double* m = &r.table[ 2 * ACN_MOTION_STRIDE ];
        EXPECT( r.status == ACN_OK && r.rep.n_rest == 7 && r.rep.n_moved == 1 && r.rep.n_none == 0 );
        const double want[ 16 ] = { 0.0, -1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, -1.2 + 3.0, -2.0, -4.0, ACN_MOTION_MOVED, 8.0, 0.0, 0.0 };
        for( int k = 0; k < 16; k++ ) EXPECT( m[ k ] == want[ k ] );
        /* the local point ( 1, 0, 0 ) of the sphere: now at pos_cur + rax_cur^T * ( 1, 0, 0 ) = ( 2, 2, 4 ), before at ( -0.2, 0, 0 ) */
        const double p[ 3 ] = { 2.0, 2.0, 4.0 };
        EXPECT( std::fabs( acn_motion_dot( m, p ) + m[ 9 ] - ( -0.2 ) ) <= 1e-15 && acn_motion_dot( m + 3, p ) + m[ 10 ] == 0.0 && acn_motion_dot( m + 6, p ) + m[ 11 ] == 0.0 );
        Result back = run( b, a, inf );                                                                            /* an infinite cap is none, and is passed on */
        EXPECT( back.status == ACN_OK && state( back, 2 ) == ACN_MOTION_MOVED && back.table[ 2 * ACN_MOTION_STRIDE + 13 ] == inf );
    }
    /* CHANGED: prm, a material member, the texture's bytes, the texture's index, sdf_kind, cycles; the envelope is ignored */
    for( int which = 0; which < 7; which++ )
    {
        Scene a = base_scene(), b = base_scene();
        acn_node& n = b.nodes[ 2 ];
        if( which == 0 ) n.prm[ 0 ] = 0.8;
        if( which == 1 ) n.transparency[ 2 ] = 0.1;
        if( which == 2 ) b.textures[ 0 ].scale = 5.0;
        if( which == 3 ) { b.textures.push_back( b.textures[ 0 ] ); n.texture = 1; }
        if( which == 4 ) n.sdf_kind = 1;
        if( which == 5 ) n.cycles = 3;
        if( which == 6 ) { n.flags = ACN_NODE_HAS_ENVELOPE; n.env_pos[ 0 ] = 1.0; n.env_radius = 2.0; n.pad_ = 1.0; n.reserved = 7; }
        quarter_turn( n, 0.0, 1.0, 0.0 );
        Result r = run( a, b );
        EXPECT( r.status == ACN_OK && state( r, 2 ) == ( which == 6 ? ACN_MOTION_MOVED : ACN_MOTION_NONE ) && r.rep.n_rest == 7 );
        if( which != 6 ) for( int k = 0; k < 16; k++ ) EXPECT( r.table[ 2 * ACN_MOTION_STRIDE + k ] == ( k == 12 ? ACN_MOTION_NONE : 0.0 ) );
    }
    /* a texture index outside the textures counts as different, and nothing outside is read */
    {
        Scene a = base_scene(), b = base_scene();
        a.nodes[ 2 ].texture = b.nodes[ 2 ].texture = 1;
        Result r = run( a, b );
        EXPECT( r.status == ACN_OK && state( r, 2 ) == ACN_MOTION_NONE );
        a.textures.clear(); b.textures.clear();
        a.nodes[ 2 ].texture = b.nodes[ 2 ].texture = 0;
        r = run( a, b );
        EXPECT( r.status == ACN_OK && state( r, 2 ) == ACN_MOTION_NONE );
    }
    /* a skewed rax, in either scene, and a NaN in it: NONE; a skew below the margin is MOVED */
    for( int which = 0; which < 4; which++ )
    {
        Scene a = base_scene(), b = base_scene();
        quarter_turn( b.nodes[ 2 ], 0.0, 1.0, 0.0 );
        if( which == 0 ) b.nodes[ 2 ].rax[ 1 ] += 1e-6;
        if( which == 1 ) a.nodes[ 2 ].rax[ 1 ] += 1e-6;
        if( which == 2 ) b.nodes[ 2 ].rax[ 8 ] = nan;
        if( which == 3 ) b.nodes[ 2 ].rax[ 2 ] += 1e-10;
        Result r = run( a, b );
        EXPECT( r.status == ACN_OK && state( r, 2 ) == ( which == 3 ? ACN_MOTION_MOVED : ACN_MOTION_NONE ) );
    }
    /* another shape: a node more, another element, another child, another type, another root */
    for( int which = 0; which < 5; which++ )
    {
        Scene a = base_scene(), b = base_scene();
        if( which == 0 ) b.nodes.push_back( node_of( ACN_SPHERE ) );
        if( which == 1 ) b.elems[ 2 ] = 2;
        if( which == 2 ) b.nodes[ 4 ].child1 = 6;
        if( which == 3 ) b.nodes[ 7 ].type = ACN_SPHERE;
        Result r;
        if( which == 4 )
        {
            r.table.assign( b.nodes.size() * ACN_MOTION_STRIDE, 7.25 );
            acn_flat_scene other = *b.c();
            other.matter_root = 0; other.light_root = 1;
            r.status = acn_motion_from_scenes_impl( a.c(), &other, 0.0, r.table.data(), &r.rep, &r.msg );
        }
        else r = run( a, b );
        EXPECT( r.status == ACN_OK && r.rep.same_shape == 0 && r.rep.n_none == b.nodes.size() && r.rep.n_rest == 0 && r.rep.n_moved == 0 );
        for( size_t i = 0; i < b.nodes.size(); i++ ) EXPECT( state( r, i ) == ACN_MOTION_NONE );
    }
    /* SCALE: the node below takes the row of the scale node; an unequal subtree makes both NONE; a pair moves node by node */
    {
        Scene a = base_scene(), b = base_scene();
        quarter_turn( b.nodes[ 3 ], 1.0, 1.0, 0.0 );
        quarter_turn( b.nodes[ 4 ], 0.0, 2.0, 0.0 ); quarter_turn( b.nodes[ 6 ], 0.0, 2.0, 0.0 );
        Result r = run( a, b, 2.0 );
        EXPECT( r.status == ACN_OK && r.rep.n_moved == 4 && r.rep.n_rest == 4 && r.rep.n_none == 0 );
        EXPECT( state( r, 3 ) == ACN_MOTION_MOVED && memcmp( &r.table[ 5 * ACN_MOTION_STRIDE ], &r.table[ 3 * ACN_MOTION_STRIDE ], sizeof( double ) * ACN_MOTION_STRIDE ) == 0 );
        EXPECT( state( r, 4 ) == ACN_MOTION_MOVED && state( r, 6 ) == ACN_MOTION_MOVED && state( r, 7 ) == ACN_MOTION_REST );
        b.nodes[ 5 ].pos[ 2 ] = 0.01;                                                                               /* the inner sphere moved inside the scaled frame */
        r = run( a, b );
        EXPECT( r.status == ACN_OK && state( r, 3 ) == ACN_MOTION_NONE && state( r, 5 ) == ACN_MOTION_NONE && r.rep.n_none == 2 && r.rep.n_moved == 2 );
        Scene c = base_scene();
        c.nodes[ 5 ].pos[ 2 ] = 0.01;                                                                               /* ... with the scale node at rest */
        r = run( a, c );
        EXPECT( r.status == ACN_OK && state( r, 3 ) == ACN_MOTION_NONE && state( r, 5 ) == ACN_MOTION_NONE && r.rep.n_rest == 6 );
    }
    /* nested scale nodes: the outermost decides */
    {
        Scene a = base_scene();
        a.nodes[ 5 ] = node_of( ACN_SCALE, 8 );
        a.nodes[ 5 ].prm[ 0 ] = a.nodes[ 5 ].prm[ 1 ] = a.nodes[ 5 ].prm[ 2 ] = 0.5;
        a.nodes.push_back( node_of( ACN_SPHERE ) );
        Scene b = a;
        quarter_turn( b.nodes[ 3 ], 1.0, 1.0, 0.0 );
        Result r = run( a, b );
        EXPECT( r.status == ACN_OK && r.rep.n_moved == 3 && state( r, 8 ) == ACN_MOTION_MOVED );
        EXPECT( memcmp( &r.table[ 8 * ACN_MOTION_STRIDE ], &r.table[ 3 * ACN_MOTION_STRIDE ], sizeof( double ) * ACN_MOTION_STRIDE ) == 0 );
        quarter_turn( b.nodes[ 5 ], 0.0, 0.0, 0.0 );                                                                /* the inner scale node turned: the subtree is unequal */
        r = run( a, b );
        EXPECT( r.status == ACN_OK && state( r, 3 ) == ACN_MOTION_NONE && state( r, 5 ) == ACN_MOTION_NONE && state( r, 8 ) == ACN_MOTION_NONE );
    }
    /* refusals: nothing is written */
    {
        Scene a = base_scene(), b = base_scene();
        std::vector< double > table( b.nodes.size() * ACN_MOTION_STRIDE, 7.25 );
        acn_motion_report rep = { 9u, 9u, 9u, 9u };
        auto untouched = [ & ] { for( double v : table ) if( v != 7.25 ) return false; return rep.n_rest == 9 && rep.same_shape == 9; };
        EXPECT( acn_motion_from_scenes_impl( nullptr, b.c(), 0.0, table.data(), &rep, &msg ) == ACN_ERR_ARG && says( msg, "prev" ) && untouched() );
        EXPECT( acn_motion_from_scenes_impl( a.c(), nullptr, 0.0, table.data(), &rep, &msg ) == ACN_ERR_ARG && says( msg, "cur" ) && untouched() );
        EXPECT( acn_motion_from_scenes_impl( a.c(), b.c(), 0.0, nullptr, &rep, &msg ) == ACN_ERR_ARG && says( msg, "out_table" ) && untouched() );
        for( double v : { nan, -1.0, -1e-300, 0.5, 0.9999999, -inf } )
            EXPECT( acn_motion_from_scenes_impl( a.c(), b.c(), v, table.data(), &rep, &msg ) == ACN_ERR_ARG && says( msg, "moved_max_history" ) && untouched() );
        { acn_flat_scene f = *b.c(); f.nodes = nullptr; EXPECT( acn_motion_from_scenes_impl( a.c(), &f, 0.0, table.data(), &rep, &msg ) == ACN_ERR_ARG && says( msg, "null" ) && untouched() ); }
        { acn_flat_scene f = *a.c(); f.elems = nullptr; EXPECT( acn_motion_from_scenes_impl( &f, b.c(), 0.0, table.data(), &rep, &msg ) == ACN_ERR_ARG && says( msg, "null" ) && untouched() ); }
        /* indices outside the scene, the same in both (so the shape is the same): a child, an element, a slice of elems, a root */
        for( int which = 0; which < 5; which++ )
        {
            Scene p = base_scene(), c = base_scene();
            for( Scene* s : { &p, &c } )
            {
                if( which == 0 ) s->nodes[ 4 ].child1 = 8;
                if( which == 1 ) s->elems[ 1 ] = -1;
                if( which == 2 ) s->nodes[ 1 ].child1 = 4;
                if( which == 3 ) s->nodes[ 3 ].child0 = 1000000;
            }
            acn_flat_scene fp = *p.c(), fc = *c.c();
            if( which == 4 ) fp.matter_root = fc.matter_root = 8;
            EXPECT( acn_motion_from_scenes_impl( &fp, &fc, 0.0, table.data(), &rep, &msg ) == ACN_ERR_ARG && says( msg, "outside" ) && untouched() );
        }
        /* a null report, empty scenes */
        EXPECT( acn_motion_from_scenes_impl( a.c(), b.c(), 1.0, table.data(), nullptr, &msg ) == ACN_OK && table[ 12 ] == 0.0 );
        Scene e, f;
        acn_flat_scene fe = *e.c(), ff = *f.c();
        fe.light_root = fe.matter_root = ff.light_root = ff.matter_root = -1;
        double none;
        EXPECT( acn_motion_from_scenes_impl( &fe, &ff, 0.0, &none, &rep, &msg ) == ACN_ERR_ARG && says( msg, "outside" ) );
    }
    /* a node both roots reach, and a cycle, end */
    {
        Scene a = base_scene();
        a.nodes[ 0 ].child0 = 0; a.nodes[ 0 ].child1 = 1;                                                           /* the light root holds node 2 too */
        a.nodes[ 7 ] = node_of( ACN_NEG, 4 );                                                                       /* 4 -> 7 -> 4 */
        Scene b = a;
        Result r = run( a, b );
        EXPECT( r.status == ACN_OK && r.rep.n_rest == 8 );
    }

    if( failures ) { printf( "%d checks failed\n", failures ); return 1; }
    printf( "ok\n" );
    return 0;
}
