/* acn_tables.h -- the scene tables of acn_scene_upload: their layouts and constants, and the host-only unit that builds them
 * (acn_tables.cpp).  No HIP header and no device code: the device side reads these through acn_device.h, the CPU tests compile
 * acn_tables.cpp with g++ and look at every table before anything reaches a device (tests/test_tables_cpu.py). */
#ifndef ACN_TABLES_H
#define ACN_TABLES_H

#include <stdint.h>
#include <stddef.h>
#include <string>
#include <vector>
#include "actinon_hip.h"
#include "acn_counts.h"   /* ACN_MAX_PATH_LEVELS */

#ifndef ACN_CSG_MAX_DEPTH
#define ACN_CSG_MAX_DEPTH   24   /* nesting of pair / neg / scale wrappers */
#endif
#ifndef ACN_CMP_MAX_DEPTH
#define ACN_CMP_MAX_DEPTH   12   /* nesting of compounds */
#endif

/* Device layout of a node: geometry only (192 B); shading properties live in GMat (104 B, read once per shading
 * point).  Built from the ABI's acn_node by acn_tables_build. */
struct GNode
{
    int32_t  type;
    uint32_t flags;
    int32_t  child0, child1;
    double   prm[ 4 ];
    double   pos[ 3 ];
    double   env_pos[ 3 ];
    double   env_radius;
    double   rax[ 9 ];
    double   surface_roughness;
    int32_t  sdf_kind, cycles;
};

struct GMat
{
    double color[ 3 ];
    double radiance;
    double refractive_index;
    double fresnel_reflectivity;
    double chromatic_reflectivity;
    double diffuse_reflectivity;
    double sigma;
    double transparency[ 3 ];
    int32_t texture;     /* index into the texture table, -1 = none */
    int32_t pad_;
};

#define ACN_GFLAG_LEAF_PAIR 0x100u      /* device-only bits of GNode.flags: a level-1 pair ... */
#define ACN_GFLAG_PAIR2     0x400u      /* ... a level-2 pair: at least one operand is a level-1 pair (machines only) */
#define ACN_GFLAG_PRUNE_LEVELS_SHIFT 12  /* bits 12 - 14: see surely_outside */
#define ACN_GFLAG_SIMPLE_COMPOUND 0x200u   /* device-only bit of GNode.flags */

#ifndef ACN_PRUNE_DEPTH
#define ACN_PRUNE_DEPTH 3
#endif

#ifndef ACN_LDS_DEPTH
#define ACN_LDS_DEPTH 3                 /* stack levels kept in LDS; deeper nesting continues in scratch */
#endif
#define ACN_LDS_LANES 256               /* block size of the kernels that provide the stack area */
/* per level and lane: a 8 B, parked normal 24 B, w 4 B, side 4 B; doubles first (alignment):
 * [ a : D x 256 ][ nx, ny, nz : 3 x D x 256 ][ w : D x 256 ][ side : D x 256 ] */
#define ACN_LDS_STACK_BYTES ( ACN_LDS_DEPTH * ACN_LDS_LANES * 40 )
/* behind the stacks: the ray origin of the lock-step machine at hand, one per lane (OrgLds): three planes of 256 doubles */
#define ACN_LDS_ORG_BYTES ( 3 * ACN_LDS_LANES * 8 )

/* One entry of a simple compound's pre-order table (simple_compound_hit): everything a visit needs -- the element's
 * envelope, its type and the two links -- in ONE 48-byte record, i.e. one memory round trip per visited node instead
 * of three dependent ones (element index -> node header -> envelope). */
struct SCEntry
{
    double  env_pos[ 3 ], env_radius;
    int32_t node;        /* node index (leaves: the object that is hit) */
    int32_t skip;        /* entry behind this element's subtree */
    int32_t type;        /* acn_node_type */
    uint32_t flags;      /* ACN_NODE_HAS_ENVELOPE | ACN_SC_SPHERE ( skip = index into sc_spheres ) | ACN_SC_ROUGH */
};
#define ACN_SC_SPHERE 0x10000u
#define ACN_SC_ROUGH  0x20000u
#define ACN_SC_BOUNDING 0x40000u   /* the upload step has verified that the envelope contains every leaf below the entry (all of them spheres) */

/* opcodes of the interval-prune programs (acn_dev_prune.h: prune_run; acn_tables.cpp: build_prune_programs) */
enum { ACN_PO_END = 0, ACN_PO_PLANE, ACN_PO_SPHERE, ACN_PO_QUAD, ACN_PO_ALL, ACN_PO_NEG, ACN_PO_AND, ACN_PO_OR, ACN_PO_ENV };
#define ACN_PO( op, node ) ( ( uint32_t )( op ) | ( ( uint32_t )( node ) << 4 ) )
#define ACN_PRUNE_STACK 5

static_assert( sizeof( GNode ) == 192, "GNode is 192 bytes on the device" );
static_assert( sizeof( GMat ) == 104, "GMat is 104 bytes on the device" );
static_assert( sizeof( SCEntry ) == 48, "SCEntry is 48 bytes on the device" );

/* the switches the table code reads; Tunables::read fills them from the environment once per upload */
struct acn_table_opts
{
    bool   no_leaf_pairs = false;         /* ACN_NO_LEAF_PAIRS */
    bool   no_pair2 = false;              /* ACN_NO_PAIR2 */
    bool   no_prune_levels = false;       /* ACN_NO_PRUNE_LEVELS */
    bool   no_simple_compounds = false;   /* ACN_NO_SIMPLE_COMPOUNDS */
    bool   no_sc_cull = false;            /* ACN_NO_SC_CULL */
    bool   no_sc_reversed = false;        /* ACN_NO_SC_REVERSED */
    size_t prune_min = 32;                /* ACN_PRUNE_MIN: nodes a CSG root element needs to get an interval-prune program */
    size_t lds_max = 0;                   /* ACN_LDS_MAX: bytes of nodes that may be staged in LDS ... */
    bool   lds_max_set = false;           /* ... given by the environment */
    bool   verbose = false;               /* ACN_VERBOSE */
};

/* everything acn_scene_upload copies to the device or keeps in the handle, as the host builds it */
struct acn_scene_tables
{
    std::vector< GNode > nodes;
    std::vector< GMat > mats;
    std::vector< int32_t > elems;         /* given order | cost order | per node: program / table offset or -1 | programs and table headers | elem_pos */
    std::vector< SCEntry > sc_table;      /* pre-order tables of the simple compounds (acn_dev_traverse.h: simple_compound_hit) */
    std::vector< double > sc_spheres;     /* ( pos, radius ) of the sphere leaves of sc_table, ( direction, 0 ) of the reversed tables */
    uint32_t prune_base = 0;              /* elems[ prune_base + node ] */
    uint32_t elem_pos_base = 0;           /* elems[ elem_pos_base + k ]: given-order position of entry k of the cost-ordered copy */
    bool prune = false;                   /* some root element has an interval-prune program or a simple-compound table */
    bool leaf_lights = true;              /* every light element is a plane / sphere */
    size_t n_lights = 1;                  /* elements of the light root */
    int n_levels = 1;                     /* path levels of the scene's trace_depth */
    size_t lds_bytes = 0, lds_stack_bytes = 0;
};

/* what the reference would abort on, plus the device limits: ACN_OK, or the code with its text in *err */
int acn_tables_validate( const acn_flat_scene* sc, int* max_csg, std::string* err );
/* the part of it that reads the render parameters alone, and the path levels of parameters it accepted: all that
 * acn_scene_set_params needs of this unit */
int acn_tables_validate_params( const acn_params* prm, std::string* err );
int acn_tables_levels( const acn_params* prm );
/* the tables of a scene that acn_tables_validate accepted */
void acn_tables_build( const acn_flat_scene* sc, const acn_table_opts& opts, acn_scene_tables* out );

#endif
