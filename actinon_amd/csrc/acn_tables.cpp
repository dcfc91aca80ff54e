/* acn_tables.cpp -- the host half of acn_scene_upload: from the ABI's acn_flat_scene to the tables every traversal shortcut of
 * the device reads (acn_tables.h).  Plain C++, no HIP: the same unit is linked into libactinon_hip.so and compiled on its own by
 * the CPU tests (tests/test_tables_cpu.py).  Compile with -ffp-contract=off: the tables hold results of floating-point sums. */
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <utility>
#include "acn_tables.h"

static bool is_pair( int type ) { return type == ACN_PAIR_INSIDE || type == ACN_PAIR_OUTSIDE; }

/* ------------------------------------------------------------------------------------------------------------------ */
/* validation: what the reference would abort on, plus the device limits */
static int csg_depth( const acn_flat_scene* sc, int node, int d, std::string& err )
{
    if( d > 4096 ) { err = "cyclic node graph"; return -1; }
    const acn_node* n = &sc->nodes[ node ];
    int m = 0;
    switch( n->type )
    {
        case ACN_PAIR_INSIDE: case ACN_PAIR_OUTSIDE:
        {
            int a = csg_depth( sc, n->child0, d + 1, err ), b = csg_depth( sc, n->child1, d + 1, err );
            if( a < 0 || b < 0 ) return -1;
            m = 1 + ( a > b ? a : b );
            break;
        }
        case ACN_NEG: case ACN_SCALE:
        {
            int a = csg_depth( sc, n->child0, d + 1, err );
            if( a < 0 ) return -1;
            m = 1 + a;
            break;
        }
        default: break;
    }
    return m;
}

static int compound_depth( const acn_flat_scene* sc, int node, int d, int* max_csg, std::string& err )
{
    if( d > 256 ) { err = "compound nesting too deep / cyclic"; return -1; }
    const acn_node* n = &sc->nodes[ node ];
    int m = 1;
    for( int k = 0; k < n->child1; k++ )
    {
        int e = sc->elems[ n->child0 + k ];
        if( sc->nodes[ e ].type == ACN_COMPOUND )
        {
            int c = compound_depth( sc, e, d + 1, max_csg, err );
            if( c < 0 ) return -1;
            if( c + 1 > m ) m = c + 1;
        }
        else
        {
            int c = csg_depth( sc, e, 0, err );
            if( c < 0 ) return -1;
            if( c > *max_csg ) *max_csg = c;
        }
    }
    return m;
}

/* the checks that read the render parameters alone (acn_scene_set_params runs these and nothing else) */
int acn_tables_validate_params( const acn_params* prm, std::string* err )
{
    auto fail = [ & ]( int code, const char* msg ) { *err = msg; return code; };
    if( prm->experimental_level != 0 ) return fail( ACN_ERR_UNSUPPORTED, "Unsupported experimental level" );   /* scene.c:1004-1007 */
    if( prm->image_height < 2 || prm->image_width < 1 ) return fail( ACN_ERR_ARG, "image size" );
    if( prm->trace_depth > 10 * ACN_MAX_PATH_LEVELS + 10 ) return fail( ACN_ERR_UNSUPPORTED, "trace_depth exceeds device path-level limit" );
    return ACN_OK;
}

/* path levels: level L shades hits at depth trace_depth - 10 L and spawns the next one while that is > 10 (scene.c:584) */
int acn_tables_levels( const acn_params* prm )
{
    const uint64_t td = prm->trace_depth;
    return prm->path_samples && td > 10 ? 1 + ( int )( ( td - 10 + 9 ) / 10 ) : 1;
}

int acn_tables_validate( const acn_flat_scene* sc, int* max_csg, std::string* err )
{
    auto fail = [ & ]( int code, const char* msg ) { *err = msg; return code; };
    if( !sc || !sc->nodes ) return fail( ACN_ERR_ARG, "null scene" );
    if( sc->abi_version != ACN_ABI_VERSION ) return fail( ACN_ERR_ARG, "abi_version mismatch" );
    if( sc->n_nodes == 0 || sc->light_root < 0 || sc->matter_root < 0 || ( uint32_t )sc->light_root >= sc->n_nodes ||
        ( uint32_t )sc->matter_root >= sc->n_nodes ) return fail( ACN_ERR_ARG, "bad root index" );
    if( sc->n_elems && !sc->elems ) return fail( ACN_ERR_ARG, "null elems" );
    if( const int st = acn_tables_validate_params( &sc->params, err ) ) return st;
    for( uint32_t i = 0; i < sc->n_nodes; i++ )
    {
        const acn_node* n = &sc->nodes[ i ];
        if( n->texture != -1 )
        {
            if( n->texture < 0 || ( uint32_t )n->texture >= sc->n_textures || !sc->textures ) return fail( ACN_ERR_ARG, "bad texture index" );
            const acn_texture* t = &sc->textures[ n->texture ];
            if( t->kind != ACN_TXM_PLAIN && t->kind != ACN_TXM_CHESS ) return fail( ACN_ERR_ARG, "unknown texture kind" );
            if( t->kind == ACN_TXM_CHESS && n->type != ACN_PLANE && n->type != ACN_SPHERE && n->type != ACN_DISTANCE )
                return fail( ACN_ERR_UNSUPPORTED, "object has no projection-function for a chess texture (objects.c:240-245)" );
        }
        switch( n->type )
        {
            case ACN_PLANE: case ACN_SPHERE: case ACN_SQUAROID: break;
            case ACN_DISTANCE:
                if( n->sdf_kind != ACN_SDF_SPHERE && n->sdf_kind != ACN_SDF_TORUS ) return fail( ACN_ERR_UNSUPPORTED, "unknown distance function" );
                break;
            case ACN_PAIR_INSIDE: case ACN_PAIR_OUTSIDE:
                if( n->child1 < 0 || ( uint32_t )n->child1 >= sc->n_nodes || sc->nodes[ n->child1 ].type == ACN_COMPOUND ) return fail( ACN_ERR_ARG, "bad pair child" );
                /* fallthrough */
            case ACN_NEG: case ACN_SCALE:
                if( n->child0 < 0 || ( uint32_t )n->child0 >= sc->n_nodes || sc->nodes[ n->child0 ].type == ACN_COMPOUND ) return fail( ACN_ERR_ARG, "bad child" );
                break;
            case ACN_COMPOUND:
                if( n->child1 < 0 || n->child0 < 0 || ( uint64_t )n->child0 + ( uint64_t )n->child1 > sc->n_elems ) return fail( ACN_ERR_ARG, "bad compound slice" );
                for( int k = 0; k < n->child1; k++ )
                {
                    int e = sc->elems[ n->child0 + k ];
                    if( e < 0 || ( uint32_t )e >= sc->n_nodes ) return fail( ACN_ERR_ARG, "bad element index" );
                }
                break;
            default: return fail( ACN_ERR_ARG, "unknown node type" );
        }
    }
    const acn_node* light = &sc->nodes[ sc->light_root ];
    if( light->type != ACN_COMPOUND || sc->nodes[ sc->matter_root ].type != ACN_COMPOUND ) return fail( ACN_ERR_ARG, "roots must be compounds" );
    for( int k = 0; k < light->child1; k++ )
    {
        int t = sc->nodes[ sc->elems[ light->child0 + k ] ].type;
        if( t == ACN_COMPOUND ) return fail( ACN_ERR_ARG, "light elements must be objects (scene.c:547)" );
        if( t != ACN_PLANE && t != ACN_SPHERE && t != ACN_PAIR_INSIDE && t != ACN_PAIR_OUTSIDE )
            return fail( ACN_ERR_NO_FOV, "light object has no fov-function (objects.c:254-258)" );
    }
    *max_csg = 0;
    int dl = compound_depth( sc, sc->light_root, 0, max_csg, *err );
    int dm = dl < 0 ? -1 : compound_depth( sc, sc->matter_root, 0, max_csg, *err );
    if( dl < 0 || dm < 0 ) return ACN_ERR_ARG;
    if( dm > ACN_CMP_MAX_DEPTH || dl > ACN_CMP_MAX_DEPTH ) return fail( ACN_ERR_UNSUPPORTED, "compound nesting exceeds device limit" );
    if( *max_csg > ACN_CSG_MAX_DEPTH ) return fail( ACN_ERR_UNSUPPORTED, "CSG nesting exceeds device limit" );
    return ACN_OK;
}

/* ------------------------------------------------------------------------------------------------------------------ */
/* ABI layout -> device layout: geometry (GNode) and shading properties (GMat) split; leaf pairs and level-2 pairs marked */
static bool simple_operand( const acn_flat_scene* scene, int32_t c )
{
    const acn_node* x = &scene->nodes[ c ];
    if( x->type == ACN_NEG ) x = &scene->nodes[ x->child0 ];
    return x->type == ACN_PLANE || x->type == ACN_SPHERE || x->type == ACN_SQUAROID;
}
static bool level1_pair( const acn_flat_scene* scene, int32_t c )
{
    const acn_node& x = scene->nodes[ c ];
    return is_pair( x.type ) && simple_operand( scene, x.child0 ) && simple_operand( scene, x.child1 );
}
static void split_nodes( const acn_flat_scene* scene, const acn_table_opts& opts, acn_scene_tables& t )
{
    t.nodes.resize( scene->n_nodes );
    t.mats.resize( scene->n_nodes );
    for( uint32_t i = 0; i < scene->n_nodes; i++ )
    {
        const acn_node& a = scene->nodes[ i ];
        GNode& g = t.nodes[ i ];
        memset( &g, 0, sizeof( g ) );
        g.type = a.type; g.flags = a.flags; g.child0 = a.child0; g.child1 = a.child1;
        if( is_pair( a.type ) && !opts.no_leaf_pairs )
        {
            if( simple_operand( scene, a.child0 ) && simple_operand( scene, a.child1 ) ) g.flags |= ACN_GFLAG_LEAF_PAIR;
            else if( ( simple_operand( scene, a.child0 ) || level1_pair( scene, a.child0 ) ) && ( simple_operand( scene, a.child1 ) || level1_pair( scene, a.child1 ) ) && !opts.no_pair2 ) g.flags |= ACN_GFLAG_PAIR2;
        }
        memcpy( g.prm, a.prm, sizeof( g.prm ) );
        memcpy( g.pos, a.pos, sizeof( g.pos ) );
        memcpy( g.env_pos, a.env_pos, sizeof( g.env_pos ) );
        g.env_radius = a.env_radius;
        memcpy( g.rax, a.rax, sizeof( g.rax ) );
        g.surface_roughness = a.surface_roughness;
        g.sdf_kind = a.sdf_kind; g.cycles = a.cycles;
        GMat& m = t.mats[ i ];
        memcpy( m.color, a.color, sizeof( m.color ) );
        m.radiance = a.radiance; m.refractive_index = a.refractive_index;
        m.fresnel_reflectivity = a.fresnel_reflectivity; m.chromatic_reflectivity = a.chromatic_reflectivity;
        m.diffuse_reflectivity = a.diffuse_reflectivity; m.sigma = a.sigma;
        memcpy( m.transparency, a.transparency, sizeof( m.transparency ) );
        m.texture = a.texture; m.pad_ = 0;
    }
}

/* surely_outside (acn_device.h) descends a pair tree up to ACN_PRUNE_DEPTH levels to test the envelopes it finds.  How many
 * levels of a node are worth reading is known here: ACN_GFLAG_PRUNE_LEVELS( flags ) = 0 if neither the node nor any pair
 * operand within three levels below it has an envelope, else 1 + the depth of the deepest such envelope -- the descent stops
 * where nothing is left to test instead of reading operands for nothing (a chain of dependent scalar loads per level). */
static int deepest_envelope( const acn_flat_scene* scene, int32_t i, int left )   /* depth of the deepest envelope within `left` levels, -1: none */
{
    const acn_node& a = scene->nodes[ i ];
    int best = ( a.flags & ACN_NODE_HAS_ENVELOPE ) ? 0 : -1;
    if( left > 0 && is_pair( a.type ) )
        for( int32_t c : { a.child0, a.child1 } ) { int d = deepest_envelope( scene, c, left - 1 ); if( d >= 0 && d + 1 > best ) best = d + 1; }
    return best;
}
static void mark_prune_levels( const acn_flat_scene* scene, const acn_table_opts& opts, acn_scene_tables& t )
{
    for( uint32_t i = 0; i < scene->n_nodes; i++ )
        t.nodes[ i ].flags |= ( opts.no_prune_levels ? 4u : ( uint32_t )( deepest_envelope( scene, ( int32_t )i, 3 ) + 1 ) ) << ACN_GFLAG_PRUNE_LEVELS_SHIFT;
}

/* elems[ 0 .. n ) as given; elems[ n .. 2n ) the same slices with each compound's elements ordered by estimated
 * test cost (any-hit occlusion queries are an OR over the elements, so their order is free; closest-hit queries
 * keep the given order because ties go to the first element, compound.c:225-243).
 * elem_pos, per entry of the cost-ordered copy: its element's position in the compound's given order (the resume words of the
 * hard-ray kernels speak of those positions, acn_device.h: root_occluded_rec); appended to elems behind everything else */
static double node_cost( const acn_flat_scene* scene, std::vector< double >& cost, int32_t i )
{
    if( cost[ i ] >= 0 ) return cost[ i ];
    const acn_node& a = scene->nodes[ i ];
    double c = 1;
    switch( a.type )
    {
        case ACN_PLANE: c = 0.5; break;
        case ACN_SPHERE: c = 1; break;
        case ACN_SQUAROID: c = 1.5; break;
        case ACN_DISTANCE: c = 60; break;            /* sphere tracing, up to `cycles` evaluations */
        case ACN_NEG: case ACN_SCALE: c = 1 + node_cost( scene, cost, a.child0 ); break;
        case ACN_PAIR_INSIDE: case ACN_PAIR_OUTSIDE: c = 2 + 1.5 * ( node_cost( scene, cost, a.child0 ) + node_cost( scene, cost, a.child1 ) ); break;
        case ACN_COMPOUND: c = 1; for( int32_t k = 0; k < a.child1; k++ ) c += node_cost( scene, cost, scene->elems[ a.child0 + k ] ); break;
        default: break;
    }
    return cost[ i ] = c;
}
static void order_by_cost( const acn_flat_scene* scene, acn_scene_tables& t, std::vector< int32_t >& elem_pos )
{
    t.elems.assign( 2 * ( size_t )scene->n_elems, 0 );
    elem_pos.assign( scene->n_elems, 0 );
    std::vector< double > cost( scene->n_nodes, -1.0 );
    for( uint32_t k = 0; k < scene->n_elems; k++ ) t.elems[ k ] = t.elems[ scene->n_elems + k ] = scene->elems[ k ];
    for( uint32_t i = 0; i < scene->n_nodes; i++ )
    {
        const acn_node& a = scene->nodes[ i ];
        if( a.type != ACN_COMPOUND || a.child1 < 2 ) continue;
        int32_t* first = t.elems.data() + scene->n_elems + a.child0;
        int32_t* at = elem_pos.data() + a.child0;
        for( int32_t k = 0; k < a.child1; k++ ) at[ k ] = k;
        std::stable_sort( at, at + a.child1, [ & ]( int32_t x, int32_t y ) { return node_cost( scene, cost, scene->elems[ a.child0 + x ] ) < node_cost( scene, cost, scene->elems[ a.child0 + y ] ); } );
        for( int32_t k = 0; k < a.child1; k++ ) first[ k ] = scene->elems[ a.child0 + at[ k ] ];
    }
}

/* elems[ 2n .. 2n + n_nodes ): per node the offset of its interval-prune program (acn_device.h: prune_run) or -1,
 * followed by the programs.  Only root elements of compounds that are CSG composites with at least
 * ACN_PRUNE_MIN nodes get one (small trees are cheaper to walk than to pre-test). */
static int32_t subtree_size( const acn_flat_scene* scene, std::vector< int32_t >& size, int32_t i )
{
    if( size[ i ] >= 0 ) return size[ i ];
    const acn_node& a = scene->nodes[ i ];
    int32_t c = 1;
    if( a.type == ACN_NEG || a.type == ACN_SCALE ) c += subtree_size( scene, size, a.child0 );
    else if( is_pair( a.type ) ) c += subtree_size( scene, size, a.child0 ) + subtree_size( scene, size, a.child1 );
    return size[ i ] = c;
}
struct PruneGen
{
    const acn_flat_scene* scene;
    std::vector< uint32_t > prog;
    int max_depth;
    /* postfix code for node i; returns the interval-stack depth it needs.  The child that needs the deeper
     * stack is emitted first (the combining ops are symmetric), which keeps balanced trees within the budget. */
    int gen( int32_t i, int depth )
    {
        const acn_node& a = scene->nodes[ i ];
        int need = 1;
        switch( a.type )
        {
            case ACN_PLANE:    prog.push_back( ACN_PO( ACN_PO_PLANE, i ) ); break;
            case ACN_SPHERE:   prog.push_back( ACN_PO( ACN_PO_SPHERE, i ) ); break;
            case ACN_SQUAROID: prog.push_back( ACN_PO( ACN_PO_QUAD, i ) ); break;
            case ACN_NEG:
            {
                const acn_node& c = scene->nodes[ a.child0 ];
                need = gen( a.child0, depth );
                bool bare_plane = c.type == ACN_PLANE && !( c.flags & ACN_NODE_HAS_ENVELOPE ) && a.child0 != 0;
                prog.push_back( ACN_PO( ACN_PO_NEG, bare_plane ? a.child0 : 0 ) );
            }
            break;
            case ACN_PAIR_INSIDE: case ACN_PAIR_OUTSIDE:
            {
                if( depth >= max_depth ) { prog.push_back( ACN_PO( ACN_PO_ALL, 0 ) ); break; }
                /* n-ary view: chains of the same pair type without envelopes in between are one intersection /
                 * union (the sets H and S do not depend on how the reference's tree is balanced); operands are
                 * combined one after the other, the one needing the deepest stack first */
                std::vector< int32_t > items, todo{ a.child1, a.child0 };
                while( !todo.empty() )
                {
                    int32_t c = todo.back(); todo.pop_back();
                    const acn_node& cn = scene->nodes[ c ];
                    if( cn.type == a.type && !( cn.flags & ACN_NODE_HAS_ENVELOPE ) ) { todo.push_back( cn.child1 ); todo.push_back( cn.child0 ); }
                    else items.push_back( c );
                }
                size_t mark = prog.size();
                std::vector< std::pair< int, std::vector< uint32_t > > > code;
                for( int32_t c : items )
                {
                    int d = gen( c, depth + 1 );
                    code.emplace_back( d, std::vector< uint32_t >( prog.begin() + mark, prog.end() ) );
                    prog.resize( mark );
                }
                std::stable_sort( code.begin(), code.end(), []( const std::pair< int, std::vector< uint32_t > >& x, const std::pair< int, std::vector< uint32_t > >& y ) { return x.first > y.first; } );
                need = code[ 0 ].first;
                for( size_t k = 0; k < code.size(); k++ )
                {
                    prog.insert( prog.end(), code[ k ].second.begin(), code[ k ].second.end() );
                    if( k > 0 )
                    {
                        prog.push_back( ACN_PO( a.type == ACN_PAIR_INSIDE ? ACN_PO_AND : ACN_PO_OR, 0 ) );
                        if( 1 + code[ k ].first > need ) need = 1 + code[ k ].first;
                    }
                }
                if( need > ACN_PRUNE_STACK ) { prog.resize( mark ); prog.push_back( ACN_PO( ACN_PO_ALL, 0 ) ); need = 1; }
            }
            break;
            default: prog.push_back( ACN_PO( ACN_PO_ALL, 0 ) ); break;
        }
        if( a.flags & ACN_NODE_HAS_ENVELOPE ) prog.push_back( ACN_PO( ACN_PO_ENV, i ) );
        return need;
    }
};
static void build_prune_programs( const acn_flat_scene* scene, const acn_table_opts& opts, acn_scene_tables& t )
{
    t.prune_base = 2 * scene->n_elems;
    t.elems.resize( 2 * ( size_t )scene->n_elems + scene->n_nodes, -1 );
    std::vector< int32_t > size( scene->n_nodes, -1 );
    PruneGen g{ scene, {}, 0 };
    const size_t max_ops = 256;
    for( uint32_t i = 0; i < scene->n_nodes; i++ )
    {
        const acn_node& c = scene->nodes[ i ];
        if( c.type != ACN_COMPOUND ) continue;
        for( int32_t k = 0; k < c.child1; k++ )
        {
            int32_t e = scene->elems[ c.child0 + k ];
            if( !is_pair( scene->nodes[ e ].type ) ) continue;
            if( ( size_t )subtree_size( scene, size, e ) < opts.prune_min || t.elems[ t.prune_base + e ] >= 0 ) continue;
            for( g.max_depth = 12; g.max_depth >= 1; g.max_depth-- )   /* the deepest expansion that fits the budget */
            {
                g.prog.clear();
                g.gen( e, 0 );
                if( g.prog.size() < max_ops ) break;
            }
            if( g.max_depth < 1 ) continue;
            g.prog.push_back( ACN_PO( ACN_PO_END, 0 ) );
            t.elems[ t.prune_base + e ] = ( int32_t )t.elems.size();
            t.prune = true;
            for( uint32_t w : g.prog ) t.elems.push_back( ( int32_t )w );
        }
    }
}

/* simple compounds (acn_device.h: simple_compound_hit): pre-order ( node, skip ) tables for root elements that
 * are compounds over nothing but compounds and simple leaves; the same per-node offset table locates them */
static bool is_simple( const acn_flat_scene* scene, std::vector< int8_t >& simple, int32_t i )
{
    if( simple[ i ] >= 0 ) return simple[ i ] != 0;
    const acn_node& a = scene->nodes[ i ];
    bool ok = a.type == ACN_PLANE || a.type == ACN_SPHERE || a.type == ACN_SQUAROID;
    if( a.type == ACN_COMPOUND )
    {
        ok = true;
        for( int32_t k = 0; k < a.child1 && ok; k++ ) ok = is_simple( scene, simple, scene->elems[ a.child0 + k ] );
    }
    simple[ i ] = ok ? 1 : 0;
    return ok;
}
struct SimpleCompounds
{
    const acn_flat_scene* scene;
    bool no_cull;
    std::vector< SCEntry >& sct;
    std::vector< double >& sc_spheres;
    std::vector< int32_t > sph_of;        /* sphere record of a leaf, flags of an entry: the reversed table reuses them */
    std::vector< uint32_t > flags_of;
    double order_dir[ 3 ];                /* along which the children of the compounds at hand come later, summed over the compounds */
    size_t n_bounding;
    static double centre( const acn_node& x, int c ) { return ( x.flags & ACN_NODE_HAS_ENVELOPE ) ? x.env_pos[ c ] : x.pos[ c ]; }
    void emit( int32_t c, bool reversed )   /* children of compound c, depth first */
    {
        const acn_node& a = scene->nodes[ c ];
        if( !reversed && a.child1 > 1 )
        {
            double mean[ 3 ] = { 0, 0, 0 };
            for( int32_t k = 0; k < a.child1; k++ ) for( int x = 0; x < 3; x++ ) mean[ x ] += centre( scene->nodes[ scene->elems[ a.child0 + k ] ], x ) / a.child1;
            for( int32_t k = 0; k < a.child1; k++ ) for( int x = 0; x < 3; x++ )
                order_dir[ x ] += ( k - 0.5 * ( a.child1 - 1 ) ) * ( centre( scene->nodes[ scene->elems[ a.child0 + k ] ], x ) - mean[ x ] );
        }
        for( int32_t kk = 0; kk < a.child1; kk++ )
        {
            const int32_t k = reversed ? a.child1 - 1 - kk : kk;
            int32_t e = scene->elems[ a.child0 + k ];
            const acn_node& en = scene->nodes[ e ];
            size_t at = sct.size();
            SCEntry rec;
            memcpy( rec.env_pos, en.env_pos, sizeof( rec.env_pos ) );
            rec.env_radius = en.env_radius; rec.node = e; rec.skip = 0; rec.type = en.type; rec.flags = en.flags & ACN_NODE_HAS_ENVELOPE;
            sct.push_back( rec );
            if( en.type == ACN_COMPOUND ) emit( e, reversed );
            sct[ at ].skip = ( int32_t )sct.size();   /* the entry behind e's subtree */
            if( reversed )
            {
                sct[ at ].flags = flags_of[ e ];
                if( en.type == ACN_SPHERE ) sct[ at ].skip = sph_of[ e ];
                continue;
            }
            if( ( rec.flags & ACN_NODE_HAS_ENVELOPE ) && !no_cull )   /* does the envelope contain every leaf below? (simple_compound_hit: CULL) */
            {
                bool inside = true;
                for( size_t j = at; j < sct.size() && inside; j++ )
                {
                    const acn_node& ln = scene->nodes[ sct[ j ].node ];
                    if( ln.type == ACN_COMPOUND ) continue;
                    if( ln.type != ACN_SPHERE ) { inside = false; break; }
                    double d2 = 0;
                    for( int x = 0; x < 3; x++ ) d2 += ( ln.pos[ x ] - en.env_pos[ x ] ) * ( ln.pos[ x ] - en.env_pos[ x ] );
                    inside = sqrt( d2 ) + fabs( ln.prm[ 0 ] ) <= fabs( en.env_radius ) * ( 1.0 - 1E-9 );
                }
                if( inside ) { sct[ at ].flags |= ACN_SC_BOUNDING; n_bounding++; }
            }
            if( en.type == ACN_SPHERE )   /* a leaf never follows its link: it names the sphere's record instead */
            {
                sph_of[ e ] = ( int32_t )( sc_spheres.size() / 4 );
                sct[ at ].skip = sph_of[ e ];
                sct[ at ].flags |= ACN_SC_SPHERE | ( en.surface_roughness > 0 ? ACN_SC_ROUGH : 0u );
                for( int x = 0; x < 3; x++ ) sc_spheres.push_back( en.pos[ x ] );
                sc_spheres.push_back( en.prm[ 0 ] );
            }
            flags_of[ e ] = sct[ at ].flags;
        }
    }
};
static void build_simple_compounds( const acn_flat_scene* scene, const acn_table_opts& opts, acn_scene_tables& t )
{
    std::vector< int8_t > simple( scene->n_nodes, -1 );
    SimpleCompounds s{ scene, opts.no_sc_cull, t.sc_table, t.sc_spheres, std::vector< int32_t >( scene->n_nodes, -1 ), std::vector< uint32_t >( scene->n_nodes, 0u ), { 0, 0, 0 }, 0 };
    size_t n_reversed = 0;
    for( int root : { scene->light_root, scene->matter_root } )
    {
        const acn_node& r = scene->nodes[ root ];
        for( int32_t k = 0; k < r.child1; k++ )
        {
            int32_t e = scene->elems[ r.child0 + k ];
            if( scene->nodes[ e ].type != ACN_COMPOUND || !is_simple( scene, simple, e ) || t.elems[ t.prune_base + e ] >= 0 ) continue;
            t.elems[ t.prune_base + e ] = ( int32_t )t.elems.size();
            t.elems.push_back( ( int32_t )s.sct.size() );     /* first entry */
            size_t first = s.sct.size();
            s.order_dir[ 0 ] = s.order_dir[ 1 ] = s.order_dir[ 2 ] = 0;
            s.emit( e, false );
            const size_t count = s.sct.size() - first;
            t.elems.push_back( ( int32_t )count );          /* entry count */
            /* the same subtree with the children of every compound in reverse order, for rays that run against the order of the
             * first (simple_compound_hit: the walk culls more the sooner it meets the near leaves); -1: none */
            const double len = sqrt( s.order_dir[ 0 ] * s.order_dir[ 0 ] + s.order_dir[ 1 ] * s.order_dir[ 1 ] + s.order_dir[ 2 ] * s.order_dir[ 2 ] );
            if( !opts.no_sc_reversed && !opts.no_sc_cull && count >= 64 && len > 0 )
            {
                t.elems.push_back( ( int32_t )s.sct.size() );
                t.elems.push_back( ( int32_t )( t.sc_spheres.size() / 4 ) );
                for( int x = 0; x < 3; x++ ) t.sc_spheres.push_back( s.order_dir[ x ] / len );
                t.sc_spheres.push_back( 0.0 );
                s.emit( e, true );
                n_reversed += count;
            }
            else { t.elems.push_back( -1 ); t.elems.push_back( 0 ); }
            t.nodes[ e ].flags |= ACN_GFLAG_SIMPLE_COMPOUND;
            t.prune = true;   /* the extras kernel variants */
        }
    }
    if( opts.verbose && s.sct.size() ) fprintf( stderr, "actinon_hip: simple compounds: %zu entries, %zu with a verified bounding envelope, %zu again in reversed order\n", s.sct.size() - n_reversed, s.n_bounding, n_reversed );
}

/* what the render path asks about the light root and the path depth */
static void light_facts( const acn_flat_scene* scene, acn_scene_tables& t )
{
    t.n_levels = acn_tables_levels( &scene->params );
    const acn_node& lr = scene->nodes[ scene->light_root ];
    t.n_lights = lr.child1 > 0 ? ( size_t )lr.child1 : 1;
    for( int k = 0; k < lr.child1; k++ )
    {
        int type = scene->nodes[ scene->elems[ lr.child0 + k ] ].type;
        if( type != ACN_PLANE && type != ACN_SPHERE ) t.leaf_lights = false;
    }
}

/* LDS plan of the machine kernels (160 KB per CU, 4 blocks of 256 lanes wanted per CU => 40 KB per block):
 *   nodes + stacks   when the node array is small (<= 8 KB: wine_glass 6 KB);
 *   nodes only       up to 40 KB (diamond): staging the per-lane node reads pays more than the stacks;
 *   stacks only      beyond (the node array stays in global memory / L2).
 * ACN_LDS_MAX (bytes of nodes that may be staged) and ACN_LDS_STACK=0|1 override. */
static void plan_lds( const acn_flat_scene* scene, const acn_table_opts& opts, acn_scene_tables& t )
{
    size_t lds_max = 40960;
    /* Round 4: nodes are staged only for scenes whose roots hold GENERIC nested compounds (hanging_lamps_in_row: compounds of
     * CSG objects) -- the one traversal left that reads nodes per lane (compound_ray_hit_dev).  The lock-step machines read
     * every node through scalar loads from global memory whatever is staged, and the leaves a root loop tests in line are
     * better off with scalar loads too: a staged node comes back through ds_read into VGPRs (1080p wine_glass 51.8 -> 50.6 ms
     * without staging, profiles/r04); the diamond's 40 KB of nodes had cost it the LDS stacks of its CSG machines. */
    bool generic_compound = false;
    for( int root : { scene->light_root, scene->matter_root } )
    {
        const acn_node& r = scene->nodes[ root ];
        for( int32_t k = 0; k < r.child1; k++ )
        {
            const int32_t e = scene->elems[ r.child0 + k ];
            if( scene->nodes[ e ].type == ACN_COMPOUND && !( t.nodes[ e ].flags & ACN_GFLAG_SIMPLE_COMPOUND ) ) generic_compound = true;
        }
    }
    if( !generic_compound ) lds_max = 0;
    if( opts.lds_max_set ) lds_max = opts.lds_max;
    size_t need = sizeof( GNode ) * ( size_t )scene->n_nodes;
    /* every machine kernel owns the stacks and the parked ray origins of its workgroup; nodes are staged in front of them
     * only if all of it fits 40 KB (four workgroups per CU) */
    t.lds_bytes = need <= lds_max && need + ACN_LDS_STACK_BYTES + ACN_LDS_ORG_BYTES <= 40960 ? need : 0;
    t.lds_stack_bytes = ACN_LDS_STACK_BYTES + ACN_LDS_ORG_BYTES;
}

void acn_tables_build( const acn_flat_scene* scene, const acn_table_opts& opts, acn_scene_tables* out )
{
    acn_scene_tables& t = *out;
    t = acn_scene_tables();
    std::vector< int32_t > elem_pos;
    split_nodes( scene, opts, t );
    mark_prune_levels( scene, opts, t );
    order_by_cost( scene, t, elem_pos );
    build_prune_programs( scene, opts, t );
    if( !opts.no_simple_compounds ) build_simple_compounds( scene, opts, t );
    t.elems.push_back( 0 );
    t.elem_pos_base = ( uint32_t )t.elems.size();
    t.elems.insert( t.elems.end(), elem_pos.begin(), elem_pos.end() );
    t.elems.push_back( 0 );
    light_facts( scene, t );
    plan_lds( scene, opts, t );
}
