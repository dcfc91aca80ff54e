/* acn_motion_host.h -- the motion table of acn_reproject_moving* without a handle and without the GPU: what the call checks of its
 * table, and acn_motion_from_scenes, which derives the table from two flat scenes (include/actinon_hip.h states the rows, the rules
 * and their order).  Plain C++, no HIP header: acn_calls.hip calls these before it touches a handle and exports the second;
 * tests/csrc/motion_cpu.cpp compiles the header on its own into a program that runs under the address and undefined-behaviour
 * sanitizers.  A check returns an acn_status and, on a refusal, the message acn_last_error will carry. */
#ifndef ACN_MOTION_HOST_H
#define ACN_MOTION_HOST_H

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "actinon_hip.h"

#define ACN_MOTION_MAX_ROWS ( ( uint64_t )1 << 31 )
#define ACN_MOTION_ORTHO_EPS 1e-9

/* what acn_reproject_moving* refuses of its table, after the checks of acn_reproject* (acn_reproject_host.h) */
static inline int acn_motion_table_check( const void* motion, uint64_t n_motion, uint64_t n, std::string* msg )
{
    if( n && !motion ) { *msg = "null argument: motion"; return ACN_ERR_ARG; }
    if( n && n_motion == 0 ) { *msg = "n_motion is 0: the motion table needs a row per node"; return ACN_ERR_ARG; }
    if( ( uintptr_t )motion % 16 ) { *msg = "the motion table is read 16 bytes at a time: align the buffer"; return ACN_ERR_ARG; }
    if( n_motion > ACN_MOTION_MAX_ROWS ) { *msg = "n_motion " + std::to_string( n_motion ) + " is above 2^31 rows"; return ACN_ERR_ARG; }
    return ACN_OK;
}

static inline double acn_motion_dot( const double* a, const double* b ) { return ( a[ 0 ] * b[ 0 ] + a[ 1 ] * b[ 1 ] ) + a[ 2 ] * b[ 2 ]; }

/* max | rax * rax^T - I | <= 1e-9; false for a NaN */
static inline bool acn_motion_orthonormal( const double* rax )
{
    for( int i = 0; i < 3; i++ )
        for( int j = 0; j < 3; j++ )
        {
            double d = acn_motion_dot( rax + 3 * i, rax + 3 * j ) - ( i == j ? 1.0 : 0.0 );
            if( d < 0 ) d = -d;
            if( !( d <= ACN_MOTION_ORTHO_EPS ) ) return false;
        }
    return true;
}

/* the texture a node names: its bytes, or null for an index outside the scene's textures */
static inline const acn_texture* acn_motion_texture( const acn_flat_scene* s, int32_t index )
{
    return ( index >= 0 && ( uint32_t )index < s->n_textures && s->textures ) ? &s->textures[ index ] : nullptr;
}

static inline bool acn_motion_texture_same( const acn_flat_scene* prev, const acn_flat_scene* cur, const acn_node& p, const acn_node& c )
{
    if( p.texture != c.texture ) return false;
    if( c.texture < 0 ) return true;
    const acn_texture* tp = acn_motion_texture( prev, p.texture );
    const acn_texture* tc = acn_motion_texture( cur, c.texture );
    return tp && tc && memcmp( tp, tc, sizeof( acn_texture ) ) == 0;
}

/* the CHANGED rule: geometry other than the frame, and the material */
static inline bool acn_motion_changed( const acn_flat_scene* prev, const acn_flat_scene* cur, const acn_node& p, const acn_node& c )
{
    const size_t mat_from = offsetof( acn_node, color ), mat_to = offsetof( acn_node, pad_ );
    return memcmp( p.prm, c.prm, sizeof( p.prm ) ) != 0 || p.sdf_kind != c.sdf_kind || p.cycles != c.cycles
        || !acn_motion_texture_same( prev, cur, p, c )
        || memcmp( ( const char* )&p + mat_from, ( const char* )&c + mat_from, mat_to - mat_from ) != 0;
}

/* the row of one node by the rules CHANGED, REST, MOVED: 16 doubles */
static inline void acn_motion_row( const acn_flat_scene* prev, const acn_flat_scene* cur, const acn_node& p, const acn_node& c,
                                   double moved_max_history, double* m )
{
    for( int k = 0; k < ACN_MOTION_STRIDE; k++ ) m[ k ] = 0.0;
    m[ 12 ] = ACN_MOTION_NONE;
    if( acn_motion_changed( prev, cur, p, c ) ) return;
    if( memcmp( p.pos, c.pos, sizeof( p.pos ) ) == 0 && memcmp( p.rax, c.rax, sizeof( p.rax ) ) == 0 ) { m[ 12 ] = ACN_MOTION_REST; return; }
    if( !acn_motion_orthonormal( p.rax ) || !acn_motion_orthonormal( c.rax ) ) return;
    for( int i = 0; i < 3; i++ )
    {
        for( int j = 0; j < 3; j++ )
            m[ 3 * i + j ] = ( p.rax[ i ] * c.rax[ j ] + p.rax[ 3 + i ] * c.rax[ 3 + j ] ) + p.rax[ 6 + i ] * c.rax[ 6 + j ];
        m[ 9 + i ] = p.pos[ i ] - acn_motion_dot( m + 3 * i, c.pos );
    }
    m[ 12 ] = ACN_MOTION_MOVED;
    m[ 13 ] = moved_max_history;
}

static inline bool acn_motion_same_shape( const acn_flat_scene* prev, const acn_flat_scene* cur )
{
    if( prev->n_nodes != cur->n_nodes || prev->n_elems != cur->n_elems || prev->light_root != cur->light_root || prev->matter_root != cur->matter_root ) return false;
    if( cur->n_elems && memcmp( prev->elems, cur->elems, sizeof( int32_t ) * cur->n_elems ) != 0 ) return false;
    for( uint32_t i = 0; i < cur->n_nodes; i++ )
    {
        const acn_node& p = prev->nodes[ i ];
        const acn_node& c = cur->nodes[ i ];
        if( p.type != c.type || p.child0 != c.child0 || p.child1 != c.child1 ) return false;
    }
    return true;
}

/* the children of node i of `s` appended to out; false: an index outside the scene */
static inline bool acn_motion_children( const acn_flat_scene* s, uint32_t i, std::vector< uint32_t >* out )
{
    const acn_node& n = s->nodes[ i ];
    auto push = [ & ]( int32_t c ) { if( c < 0 || ( uint32_t )c >= s->n_nodes ) return false; out->push_back( ( uint32_t )c ); return true; };
    switch( n.type )
    {
        case ACN_PAIR_INSIDE: case ACN_PAIR_OUTSIDE: return push( n.child0 ) && push( n.child1 );
        case ACN_NEG: case ACN_SCALE: return push( n.child0 );
        case ACN_COMPOUND:
            if( n.child1 == 0 ) return true;
            if( n.child1 < 0 || n.child0 < 0 || ( uint64_t )n.child0 + ( uint64_t )n.child1 > s->n_elems ) return false;
            for( int32_t k = 0; k < n.child1; k++ ) if( !push( s->elems[ n.child0 + k ] ) ) return false;
            return true;
        default: return true;
    }
}

static inline int acn_motion_from_scenes_impl( const acn_flat_scene* prev, const acn_flat_scene* cur, double moved_max_history, double* out_table,
                                               acn_motion_report* report, std::string* msg )
{
    if( !prev ) { *msg = "null argument: prev"; return ACN_ERR_ARG; }
    if( !cur ) { *msg = "null argument: cur"; return ACN_ERR_ARG; }
    if( !out_table ) { *msg = "null argument: out_table"; return ACN_ERR_ARG; }
    if( ( prev->n_nodes && !prev->nodes ) || ( prev->n_elems && !prev->elems ) ) { *msg = "null argument: prev has no nodes or elems"; return ACN_ERR_ARG; }
    if( ( cur->n_nodes && !cur->nodes ) || ( cur->n_elems && !cur->elems ) ) { *msg = "null argument: cur has no nodes or elems"; return ACN_ERR_ARG; }
    if( !( moved_max_history >= 0 ) || ( moved_max_history > 0 && moved_max_history < 1 ) )
    {
        *msg = "moved_max_history is not 0 and not a number >= 1";
        return ACN_ERR_ARG;
    }
    const uint32_t n = cur->n_nodes;
    acn_motion_report rep = { 0u, 0u, 0u, 0u };
    rep.same_shape = acn_motion_same_shape( prev, cur ) ? 1u : 0u;
    /* SCALE needs the tree: the outermost ACN_SCALE ancestor of every node, -1 for none.  Walked before anything is written, so that
     * a refusal writes nothing.  A node is visited once: the first path from a root decides */
    std::vector< int32_t > outer( n, -1 );
    if( rep.same_shape )
    {
        std::vector< char > seen( n, 0 );
        std::vector< uint32_t > stack, kids;
        for( int32_t root : { cur->light_root, cur->matter_root } )
        {
            if( root < 0 || ( uint32_t )root >= n ) { *msg = "a root index outside cur"; return ACN_ERR_ARG; }
            if( !seen[ root ] ) { seen[ root ] = 1; stack.push_back( ( uint32_t )root ); }
        }
        while( !stack.empty() )
        {
            const uint32_t i = stack.back();
            stack.pop_back();
            kids.clear();
            if( !acn_motion_children( cur, i, &kids ) ) { *msg = "a child or element index outside cur"; return ACN_ERR_ARG; }
            const int32_t below = outer[ i ] >= 0 ? outer[ i ] : cur->nodes[ i ].type == ACN_SCALE ? ( int32_t )i : -1;
            for( uint32_t k : kids )
                if( !seen[ k ] ) { seen[ k ] = 1; outer[ k ] = below; stack.push_back( k ); }
        }
    }
    for( uint32_t i = 0; i < n; i++ )
    {
        double* m = out_table + ( size_t )i * ACN_MOTION_STRIDE;
        if( rep.same_shape ) acn_motion_row( prev, cur, prev->nodes[ i ], cur->nodes[ i ], moved_max_history, m );
        else { for( int k = 0; k < ACN_MOTION_STRIDE; k++ ) m[ k ] = 0.0; m[ 12 ] = ACN_MOTION_NONE; }
    }
    if( rep.same_shape )
    {
        /* SCALE: is everything strictly below an outermost scale node equal?  then its row, else NONE for the subtree and the node */
        std::vector< char > unequal( n, 0 );
        for( uint32_t i = 0; i < n; i++ )
        {
            if( outer[ i ] < 0 ) continue;
            const acn_node& p = prev->nodes[ i ];
            const acn_node& c = cur->nodes[ i ];
            if( memcmp( &p, &c, sizeof( acn_node ) ) != 0 || !acn_motion_texture_same( prev, cur, p, c ) ) unequal[ outer[ i ] ] = 1;
        }
        for( uint32_t i = 0; i < n; i++ )
        {
            if( outer[ i ] < 0 ) continue;
            double* m = out_table + ( size_t )i * ACN_MOTION_STRIDE;
            if( unequal[ outer[ i ] ] ) { for( int k = 0; k < ACN_MOTION_STRIDE; k++ ) m[ k ] = 0.0; m[ 12 ] = ACN_MOTION_NONE; }
            else memcpy( m, out_table + ( size_t )outer[ i ] * ACN_MOTION_STRIDE, sizeof( double ) * ACN_MOTION_STRIDE );
        }
        for( uint32_t i = 0; i < n; i++ )
            if( unequal[ i ] )
            {
                double* m = out_table + ( size_t )i * ACN_MOTION_STRIDE;
                for( int k = 0; k < ACN_MOTION_STRIDE; k++ ) m[ k ] = 0.0;
                m[ 12 ] = ACN_MOTION_NONE;
            }
    }
    for( uint32_t i = 0; i < n; i++ )
    {
        const double state = out_table[ ( size_t )i * ACN_MOTION_STRIDE + 12 ];
        if( state == ACN_MOTION_REST ) rep.n_rest++;
        else if( state == ACN_MOTION_MOVED ) rep.n_moved++;
        else rep.n_none++;
    }
    if( report ) *report = rep;
    return ACN_OK;
}

#endif
