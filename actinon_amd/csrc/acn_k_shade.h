/* acn_k_shade.h -- k_shade with the body of its launch wrappers: included by the k_shade_*.hip units alone (acn_launch.h) */
#ifndef ACN_K_SHADE_H
#define ACN_K_SHADE_H

#include "acn_queues.h"
#include "acn_launch.h"
#include "acn_variant.h"

/* ---- LCG jump-ahead: x -> a^(2^K) x + c_K in one step, constants folded at compile time ---- */
struct LcgStep { uint64_t a, c; };

constexpr LcgStep lcg_pow2( int k )
{
    LcgStep s = { ACN_LCG00_A, ACN_LCG00_C };
    for( int i = 0; i < k; i++ ) { s.c = ( s.a + 1 ) * s.c; s.a = s.a * s.a; }
    return s;
}

template< int K > DEV uint64_t lcg_jump_pow2( uint64_t x )
{
    constexpr LcgStep s = lcg_pow2( K );
    return s.a * x + s.c;
}

/* jump by 2*sub draws for sub < 64 */
DEV uint64_t lcg_jump_lane( uint64_t x, int sub )
{
    if( sub & 1 )  x = lcg_jump_pow2< 1 >( x );
    if( sub & 2 )  x = lcg_jump_pow2< 2 >( x );
    if( sub & 4 )  x = lcg_jump_pow2< 3 >( x );
    if( sub & 8 )  x = lcg_jump_pow2< 4 >( x );
    if( sub & 16 ) x = lcg_jump_pow2< 5 >( x );
    if( sub & 32 ) x = lcg_jump_pow2< 6 >( x );
    return x;
}

/* ------------------------------------------------------------------------------------------------------------------ */
/* k_shade: the two sample loops of a diffuse shading point, LPT lanes per task */

template< int LPT > DEV double group_sum( double v )
{
    for( int off = LPT / 2; off > 0; off >>= 1 ) v += __shfl_xor( v, off, 64 );
    return v;
}

template< int LPT > DEV uint64_t lcg_stride( uint64_t x )   /* jump by 2*LPT draws */
{
    if( LPT == 64 ) return lcg_jump_pow2< 7 >( x );
    if( LPT == 16 ) return lcg_jump_pow2< 5 >( x );
    if( LPT == 4 )  return lcg_jump_pow2< 3 >( x );
    return lcg_jump_pow2< 1 >( x );
}

/* Task frames.  A shading point's sample loops run 13 (200 samples on 16 lanes) to hundreds of rounds over ~40 doubles that do
 * not change from round to round: the surface frame, the Oren-Nayar constants, the light's sampling frame, position, radiance and
 * colour, the throughput.  Held in registers next to a round's own temporaries they do not fit the 128 VGPRs k_shade runs best
 * with, and what the allocator spills is exactly these values: round 3's kernel reloaded ~16 of them from SCRATCH in every round
 * (1.95e8 vector-memory instructions per 1080p frame at ~590 cycles each, 17 GB of spill writes; profiles/r03/NOTES.md section 1).
 * All LPT lanes of a task hold the SAME values, so they live once per task in LDS instead: the lane with sub == 0 writes the
 * frame when the task (and each light) is set up, and a round reads a value where it needs it -- a broadcast ds_read, ~64 cycles,
 * no VMEM slot, no register held across the round.  The accesses are volatile: the compiler neither keeps a value in a register
 * across uses nor moves a read above the write of another lane (LDS operations of one wave execute in program order).
 * Narrow classes (LPT < 16: 64 or 256 tasks per workgroup) keep the frame in registers as before: they are 3 % of the time. */
enum
{
    TF_SURFACE_D = 0, TF_RAY_PRJ = 3, TF_SIN_I = 6, TF_COS_I, TF_TAN_I, TF_THETA_I, TF_ON_A, TF_ON_B, TF_DIFF_I,
    TF_CON = 13,          /* 9: rows of the transposed sampling frame (src_con of the light at hand, then out_con of the path loop) */
    TF_CYL_HGT = 22, TF_LIGHT_POS = 23, TF_RADIANCE = 26,
    TF_SCALE = 27,        /* 3: direct loop: Tc * light_color * ( 2 cyl_hgt / direct_samples ), what a deferred sample's c is multiplied with;
                                path loop: Tchild = Tc * ( 2 / path_samples ) */
    TF_N = 30,
    /* the batched set-up (k_shade, BATCHED) sets a task up on one lane and runs its loops on a group of lanes, so what a group
     * holds in registers across a task otherwise is part of the frame: the origin, the luminance so far, the light's colour and
     * the loop's normalisation, the state of the LCG stream the loop at hand starts from, the cone cull's skip word, the task slot.
     * 43 doubles: the 16 frames of a batch, and the four of a sub-step, start in distinct LDS banks */
    TF_POS = 30, TF_LUM = 33, TF_LIGHT_COLOR = 36, TF_NORM = 39, TF_RV, TF_SKIP, TF_SLOT, TF_BATCH_N
};
template< bool IN_LDS > struct TaskFrame;
template<> struct TaskFrame< true >
{
    volatile double ACN_LDS* p;
    DEV double get( int k ) const { return p[ k ]; }
    DEV V3 get3( int k ) const { return mk( p[ k ], p[ k + 1 ], p[ k + 2 ] ); }
    DEV void set( bool writer, int k, double v ) { if( writer ) p[ k ] = v; }
    DEV void set3( bool writer, int k, V3 v ) { if( writer ) { p[ k ] = v.x; p[ k + 1 ] = v.y; p[ k + 2 ] = v.z; } }
    DEV uint64_t getu( int k ) const { return ( ( volatile uint64_t ACN_LDS* )p )[ k ]; }   /* a slot that holds 64 bits as they are */
    DEV void setu( int k, uint64_t v ) { ( ( volatile uint64_t ACN_LDS* )p )[ k ] = v; }
    /* the writes of the task's first lane are visible to the reads of the others: same wave, program order; the fence keeps the
     * compiler from moving memory operations across */
    DEV void publish() const { __builtin_amdgcn_fence( __ATOMIC_SEQ_CST, "wavefront" ); __builtin_amdgcn_wave_barrier(); }
};
template<> struct TaskFrame< false >
{
    double r[ TF_N ];
    DEV double get( int k ) const { return r[ k ]; }
    DEV V3 get3( int k ) const { return mk( r[ k ], r[ k + 1 ], r[ k + 2 ] ); }
    DEV void set( bool, int k, double v ) { r[ k ] = v; }
    DEV void set3( bool, int k, V3 v ) { r[ k ] = v.x; r[ k + 1 ] = v.y; r[ k + 2 ] = v.z; }
    DEV void publish() const {}
};
template< class F > DEV M3 frame_con( const F& f )
{
    M3 m;
    m.x = f.get3( TF_CON ); m.y = f.get3( TF_CON + 3 ); m.z = f.get3( TF_CON + 6 );
    return m;
}
template< class F > DEV void frame_set_con( F& f, bool w, const M3& m ) { f.set3( w, TF_CON, m.x ); f.set3( w, TF_CON + 3, m.y ); f.set3( w, TF_CON + 6, m.z ); }

/* The root positions a wave's occlusion tests still visit for the light at hand (root_occluded_fast's POS).  root_cone_cull
 * gives every task the positions no ray of its cone can hit; a position that every lane of the wave skips is visited by no
 * sample, and on the wine glass most floor points skip them all.  So the positions some lane wants are formed once per light
 * -- wave-uniform, bit i: position i < 64; positions from 64 on are always visited -- and the sample loop walks the set bits
 * with scalar code instead of testing each lane's skip bit at every position.  A lane still tests a position only if its
 * own skip bit is clear, returns at its first occluding element and ORs the same resume bits: the set only leaves out trips
 * in which no lane did anything.  The root node's own fields are read here once as well. */
struct RootSet
{
    uint64_t want;
    int first_, count_;
    bool env_;
    template< class NP > DEV bool env( NP ) const { return env_; }
    template< class NP > DEV int first( NP ) const { return first_; }
    template< class NP > DEV int count( NP ) const { return count_; }
    DEV bool none() const { return want == 0 && count_ <= 64; }
    DEV int begin() const { return want ? ( int )__builtin_ctzll( want ) : 64; }
    DEV int next( int i )
    {
        if( i >= 64 ) return i + 1;
        want &= want - 1;
        return begin();
    }
};
/* (the narrow classes run one or two rounds per light, too few to earn the set back: they keep RootAll, and so do the PRUNE
 * variants: WAVE_LOOPS in k_shade) */
template< bool WAVE_SET, class SC > DEV auto root_set( const SC& sc, int cmp, uint64_t skip )
{
    if constexpr( !WAVE_SET ) return RootAll();
    else
    {
        auto o = &sc.nodes[ cmp ];
        RootSet s;
        s.env_ = node_has_env( o ); s.first_ = o->child0; s.count_ = o->child1;
        s.want = 0;
        const int n = s.count_ < 64 ? s.count_ : 64;
        for( int i = 0; i < n; i++ )
            if( __ballot( !( ( skip >> i ) & 1ull ) ) != 0ull ) s.want |= 1ull << i;
        return s;
    }
}

/* The cap sample of the wide classes: v_random_sphere_cap (acn_device.h) with the quadrant of acn_sincos (acn_detmath.h) picked
 * by selects.  The lanes of a wave fall into all four quadrants, so the switch runs every arm under its own exec mask; here the
 * swap is bit 0 of n, the sign of the sine bit 1 of n and the sign of the cosine bit 1 of n + 1 -- four conditional moves.
 * Same reduction, same kernels, and a negation is exact: the same bits.  (k_shade< 4 > got slower with it, 1.579 -> 1.600 ms, and
 * the narrow classes keep the switch: profiles/r22/NOTES.md.) */
DEV void sincos_select( double x, double* s, double* c )
{
    double y0, y1;
    const int n = acn_rem_pio2( acn_fabs( x ), &y0, &y1 );
    const double ks = acn_k_sin( y0, y1 ), kc = acn_k_cos( y0, y1 );
    double ss = ( n & 1 ) ? kc : ks, cc = ( n & 1 ) ? ks : kc;
    ss = ( n & 2 ) ? -ss : ss;
    cc = ( ( n + 1 ) & 2 ) ? -cc : cc;
    *s = ( x < 0 ) ? -ss : ss;
    *c = cc;
}
template< bool SELECT > DEV V3 shade_sphere_cap( uint64_t* rv, double h )
{
    if constexpr( !SELECT ) return v_random_sphere_cap( rv, h );
    else
    {
        V3 v;
        double phi = 2.0 * ACN_PI * f3_rnd1( rv );
        v.z = 1.0 - f3_rnd1( rv ) * h;
        double scale = acn_sqrt( 1.0 - v.z * v.z );
        double s, c;
        sincos_select( phi, &s, &c );
        v.x = s * scale;
        v.y = c * scale;
        return v;
    }
}

/* What runs before a task's sample loops.  Both forms of k_shade's step use it, the plain step and the batched form (BATCHED): this
 * is the one place it is defined.  The three set-ups are text, as the sample loops are (acn_k_shade_direct_loop.h): a form
 * compiles from the tokens it would have written out, and a change to one form's step leaves the other's code object alone; through
 * DEV functions or lambdas shared by the two forms it did not.  f is the frame that is set up and w whether
 * the lane writes it: fr_ and writer in the plain step, the frame of the lane's own task and true in the batched form.
 * ACN_SHADE_TASK_SETUP: the task's own values, the surface frame and the Oren-Nayar constants.  In scope: t (the DTask). */
#define ACN_SHADE_TASK_SETUP( f, w ) \
    { \
        const V3 surface_d = ldc( t.surface_d ); \
        f.set3( w, TF_SURFACE_D, surface_d ); \
        f.set3( w, TF_RAY_PRJ, ldc( t.ray_projection ) ); \
        const double theta_i = t.theta_i; \
        double sin_i = 0, cos_i = 1;   /* loop invariant half of the Oren-Nayar term */ \
        if( t.on_b > 0 ) acn_sincos( theta_i, &sin_i, &cos_i ); \
        f.set( w, TF_SIN_I, sin_i ); f.set( w, TF_COS_I, cos_i ); \
        f.set( w, TF_TAN_I, cos_i > 0 ? sin_i / cos_i : 0.0 );   /* direct-light loop only, and only where cos_i > weight > 0 */ \
        f.set( w, TF_THETA_I, theta_i ); \
        f.set( w, TF_ON_A, t.on_a ); f.set( w, TF_ON_B, t.on_b ); \
        f.set( w, TF_DIFF_I, t.diffuse_intensity ); \
    }
/* ACN_SHADE_LIGHT_SETUP: a light's, scene.c:542-555: the sampling frame, the root elements the cone cull leaves, colour and
 * normalisation.  In scope: t, pos, light_idx, light_src and light_mat (the light's node and material), direct_samples, and the
 * scene (sc, scp).  It assigns skip, light_color and norm. */
#define ACN_SHADE_LIGHT_SETUP( f, w ) \
    { \
        V3 fov_d; double cos_rs; \
        obj_fov_dev( light_src, pos, &fov_d, &cos_rs ); \
        const M3 src_frame = m_con_z( fov_d ); \
        const double cyl_hgt = 1 - cos_rs; \
        /* root elements no shadow ray of this loop can reach (all of them lie in the light's sampling cone; src_frame.z is \
         * the axis the cap samples are drawn around) */ \
        skip = root_cone_cull( scp, sc.matter_root, pos, src_frame.z, 1.0 - cyl_hgt ); \
        const V3 light_pos = ld3( light_src->pos ); \
        light_color = obj_color_dev( sc, light_idx, light_pos );   /* scene.c:552 */ \
        norm = 2.0 * cyl_hgt / direct_samples; \
        frame_set_con( f, w, m_transposed( src_frame ) ); \
        f.set( w, TF_CYL_HGT, cyl_hgt ); \
        f.set3( w, TF_LIGHT_POS, light_pos ); \
        f.set( w, TF_RADIANCE, light_mat->radiance ); \
        const V3 Tc = ldc( t.Tc ); \
        f.set3( w, TF_SCALE, mk( Tc.x * ( light_color.x * norm ), Tc.y * ( light_color.y * norm ), Tc.z * ( light_color.z * norm ) ) ); \
    }
/* ACN_SHADE_PATH_SETUP: the path loop's, scene.c:584-595.  In scope: t, and norm, 2 / path_samples. */
#define ACN_SHADE_PATH_SETUP( f, w ) \
    { \
        frame_set_con( f, w, m_transposed( m_con_z( f.get3( TF_SURFACE_D ) ) ) ); \
        f.set3( w, TF_SCALE, v_mlf( ldc( t.Tc ), norm ) ); \
    }
/* the samples of a loop: per_unit is the scene's direct_samples or path_samples */
DEV uint64_t shade_sample_count( double per_unit, double diffuse_intensity )
{
    const uint64_t n = ( uint64_t )( per_unit * diffuse_intensity );
    return n == 0 ? ( uint64_t )1 : n;
}
/* (shade_path_limit, the any-hit limit of a dark path ray: acn_queues.h, beside F3_BIG: k_hard_shadow reads it too) */

/* LEAF_LIGHTS: every light is a plane / sphere / squaroid-free leaf, so the kernel contains no call into the CSG
 * machine at all (the usual case); otherwise the light hit goes through the generic element test.
 * The tasks are idx[ 0 .. min( p_counts[ QC_CLASS0 + cls ], task_cap ) ) (dead entries skipped); the persistent waves of
 * the grid fetch them through the cursor of the class. */
template< int LPT, bool COUNT, bool LEAF_LIGHTS, bool PRUNE >
__global__ __launch_bounds__( 256, ACN_SHADE_WAVES )
void k_shade( ACN_SCENE_PARAMS, const DTask* __restrict__ tasks, const uint32_t* __restrict__ idx, int cls, uint32_t task_cap, uint32_t fetch_batch,
              HitRec* __restrict__ p_children, uint32_t child_cap, HardShadow* __restrict__ p_hard_shadow,
              HardPath* __restrict__ p_hard_path, uint32_t hs_cap, uint32_t hard_cap, uint32_t* __restrict__ p_counts, uint32_t shard_rank, uint32_t shard_world,
              unsigned long long* __restrict__ accum, unsigned long long* __restrict__ counters )
{
    ACN_CHUNK_STATES
    ACN_CHUNK_FLAGS_LOAD
    ACN_SCENE_VIEW
    const auto scp = scene_view< PRUNE >( sc, sc.nodes );   /* the scene as the two root-traversal fast paths see it */
    const ChunkP cs = ACN_CHUNKS_OF_WAVE;                   /* [0] hard shadow, [1] hard path, [2] children */
    chunks_init( cs );
    ACN_PHASE_INIT
    constexpr int G = 64 / LPT;
    constexpr bool FRAME_IN_LDS = LPT >= 16;
    /* the wave's root set and the cap sample by selects (RootSet, shade_sphere_cap above): the wide classes without the interval
     * stack of the PRUNE variants, which spilled more with them and got slower (many_spheres +1 %, profiles/r22/NOTES.md) */
    constexpr bool WAVE_LOOPS = FRAME_IN_LDS && !PRUNE;
    /* Batched set-up.  What runs before a task's sample loops -- its frame, and per light the sampling frame, the cone cull and the
     * colour -- is the same in all LPT lanes of its group: with G tasks per step a wave issues all of it for G distinct values.  Here
     * a wave takes B tasks at a time and sets them up one task per lane, light by light; the sub-steps q = 0 .. ceil( got / G ) - 1
     * then run the loops of task q * G + grp on group grp against that task's frame, as a step does otherwise.  Per task the same
     * arithmetic on the same operands in the same order: lights in their order, then the path loop; its LCG stream; its samples on
     * lanes ( j - j_lo ) % LPT.  Only the order of the records in the three output queues changes.  Class 16 alone: a task of class
     * 64 runs dozens of rounds per set-up, and 16 of them in one fetch would unbalance the end of a launch (balanced_batch). */
    constexpr bool BATCHED = WAVE_LOOPS && LPT == 16;
    constexpr int B = BATCHED ? 16 : G;   /* tasks a wave takes at a time */
    __shared__ __attribute__( ( aligned( 16 ) ) ) double acn_task_frames[ BATCHED ? 4 * B * TF_BATCH_N : FRAME_IN_LDS ? ( 256 / LPT ) * TF_N : 1 ];
    const int lane = threadIdx.x & 63;
    const int sub = lane % LPT;
    const int grp = lane / LPT;
    const bool writer = sub == 0;
    TaskFrame< FRAME_IN_LDS > fr_;
    if constexpr( FRAME_IN_LDS ) fr_.p = ( volatile double ACN_LDS* )acn_task_frames + ( threadIdx.x / LPT ) * TF_N;
    const TaskFrame< FRAME_IN_LDS >& F = fr_;
    Cnt< COUNT > cnt;
    cnt.clear();
    uint32_t n_tasks = p_counts[ QC_CLASS0 + cls ];
    n_tasks = n_tasks < task_cap ? n_tasks : task_cap;
    n_tasks = ( uint32_t )__builtin_amdgcn_readfirstlane( ( int )n_tasks );
    ACN_LEAVE_IF_CHUNK_IS_LOST
    fetch_batch = balanced_batch( n_tasks, fetch_batch, ( uint32_t )B );
    uint32_t n_hs = 0, n_hp = 0, n_ch = 0;   /* statistics: records written by this lane */
    auto kill_hs = [ p_hard_shadow ]( uint32_t k ) { p_hard_shadow[ k ].pixel = ACN_INVALID; };
    auto kill_hp = [ p_hard_path ]( uint32_t k ) { p_hard_path[ k ].pixel = ACN_INVALID; };
    auto kill_ch = [ p_children ]( uint32_t k ) { p_children[ k ].pixel = ACN_INVALID; };

    FetchRange fr;
    range_init( fr, n_tasks > 0 );
    /* persistent waves, batched: B tasks per step, in sub-steps of G; fetched fetch_batch at a time through the class's cursor.
     * (The two forms share the set-up, ACN_SHADE_TASK_SETUP and what follows it above, and the sample loops as text,
     * acn_k_shade_direct_loop.h and acn_k_shade_path_loop.h.) */
    if constexpr( BATCHED )
    {
        /* What is set up before the loops (ACN_SHADE_TASK_SETUP and what follows it, above), into the frame f of the lane's own task.
         * The task's and a light's set-up stay lambdas here: with the text where they are called, instructions of this form moved */
        auto task_setup = [ & ]( TaskFrame< FRAME_IN_LDS >& f, const DTask ACN_CONST& t ) { ACN_SHADE_TASK_SETUP( f, true ) };
        auto light_setup = [ & ]( TaskFrame< FRAME_IN_LDS >& f, const DTask ACN_CONST& t, const V3 pos, const uint64_t direct_samples, const int light_idx,
                                  uint64_t& skip, V3& light_color, double& norm )
        {
            NodeP light_src = &sc.nodes[ light_idx ];
            MatP light_mat = &sc.mats[ light_idx ];
            ACN_SHADE_LIGHT_SETUP( f, true )
        };

        volatile double ACN_LDS* const wave_frames = ( volatile double ACN_LDS* )acn_task_frames + ( threadIdx.x >> 6 ) * ( B * TF_BATCH_N );
        TaskFrame< true > mine;   /* the frame of the task this lane sets up: lanes 0 .. B - 1 */
        mine.p = wave_frames + ( lane % B ) * TF_BATCH_N;
        NodeP light = &sc.nodes[ sc.light_root ];
        const int n_lights = light->child1;
        for( ;; )
        {
            uint32_t base = 0;
            const uint32_t got = range_take( fr, p_counts + QC_CUR_SHADE0 + cls, fetch_batch, n_tasks, ( uint32_t )B, &base );
            if( got == 0 ) break;
            const uint32_t n_sub = ( got + G - 1 ) / G;
            /* task phase: lane k < got has entry base + k of the index list; a dead entry leaves a dead frame */
            uint32_t slot = ACN_INVALID;
            if( ( uint32_t )lane < got ) slot = ( ( ElemP )( const void* )idx )[ base + lane ];
            const bool setup = slot != ACN_INVALID;
            const DTask ACN_CONST& t = ( ( const DTask ACN_CONST* )tasks )[ setup ? slot : 0u ];   /* read under `setup` alone */
            if( lane < B ) mine.setu( TF_SLOT, slot );
            if( setup )
            {
                task_setup( mine, t );
                mine.set3( true, TF_POS, ldc( t.pos ) );
                mine.set3( true, TF_LUM, mk( 0, 0, 0 ) );   /* lum_l of scene.c:539 */
                mine.setu( TF_RV, t.rv );
            }
            ACN_LAP( PH_FETCH );

            /* ---- direct light, scene.c:542-581 ---- */
            for( int li = 0; li < n_lights; li++ )
            {
                const int light_idx = __builtin_amdgcn_readfirstlane( sc.elems[ light->child0 + li ] );
                NodeP light_src = &sc.nodes[ light_idx ];
                if( setup )
                {
                    cnt.cost( ACN_F_FOV + ACN_F_FRAME );   /* per task and light */
                    const uint64_t direct_samples = shade_sample_count( sc.prm.direct_samples, mine.get( TF_DIFF_I ) );
                    if( li > 0 ) mine.setu( TF_RV, lcg00_jump( mine.getu( TF_RV ), 2 * direct_samples ) );   /* behind the loop of light li - 1 */
                    uint64_t skip; V3 light_color; double norm;
                    light_setup( mine, t, mine.get3( TF_POS ), direct_samples, light_idx, skip, light_color, norm );
                    mine.setu( TF_SKIP, skip );
                    mine.set3( true, TF_LIGHT_COLOR, light_color );
                    mine.set( true, TF_NORM, norm );
                }
                mine.publish();
                ACN_LAP( PH_LIGHT_SETUP );
                for( uint32_t q = 0; q < n_sub; q++ )
                {
                    fr_.p = wave_frames + ( q * G + grp ) * TF_BATCH_N;
                    const uint32_t q_slot = ( uint32_t )F.getu( TF_SLOT );
                    if( q_slot == ACN_INVALID ) continue;
                    const DTask ACN_CONST& t = ( ( const DTask ACN_CONST* )tasks )[ q_slot ];   /* the group's task, as the loop names it */
                    const V3 pos = F.get3( TF_POS );
                    const bool oren_nayar = F.get( TF_ON_B ) > 0;
                    const uint64_t skip = F.getu( TF_SKIP ), rv = F.getu( TF_RV );
                    const uint64_t direct_samples = shade_sample_count( sc.prm.direct_samples, F.get( TF_DIFF_I ) );
                    const auto root_at = root_set< true >( scp, sc.matter_root, skip );
#include "acn_k_shade_direct_loop.h"
                    s = group_sum< LPT >( s );
                    const double f = s * F.get( TF_NORM );
                    if( writer )
                    {
                        V3 lum = F.get3( TF_LUM );
                        const V3 light_color = F.get3( TF_LIGHT_COLOR );
                        lum.x += light_color.x * f; lum.y += light_color.y * f; lum.z += light_color.z * f;
                        fr_.set3( true, TF_LUM, lum );
                    }
                    ACN_LAP( PH_SHADE );
                }
                fr_.publish();
            }

            /* ---- path tracing, scene.c:584-621 ---- */
            if( sc.prm.path_samples )
            {
                const V3 bg = ld3( sc.prm.background_color );
                const double path_limit = shade_path_limit( sc.prm.max_path_length );
                if( setup && t.depth > 10 )
                {
                    cnt.cost( ACN_F_FRAME );
                    const double diffuse_intensity = mine.get( TF_DIFF_I );
                    if( n_lights > 0 ) mine.setu( TF_RV, lcg00_jump( mine.getu( TF_RV ), 2 * shade_sample_count( sc.prm.direct_samples, diffuse_intensity ) ) );
                    const double norm = 2.0 / shade_sample_count( sc.prm.path_samples, diffuse_intensity );
                    ACN_SHADE_PATH_SETUP( mine, true )
                    mine.set( true, TF_NORM, norm );
                }
                mine.publish();
                ACN_LAP( PH_PATH_SETUP );
                for( uint32_t q = 0; q < n_sub; q++ )
                {
                    fr_.p = wave_frames + ( q * G + grp ) * TF_BATCH_N;
                    const uint32_t q_slot = ( uint32_t )F.getu( TF_SLOT );
                    if( q_slot == ACN_INVALID ) continue;
                    const DTask ACN_CONST& t = ( ( const DTask ACN_CONST* )tasks )[ q_slot ];
                    if( !( t.depth > 10 ) ) continue;
                    const V3 pos = F.get3( TF_POS );
                    const bool oren_nayar = F.get( TF_ON_B ) > 0;
                    const double diffuse_intensity = F.get( TF_DIFF_I );
                    const uint64_t rv = F.getu( TF_RV );
                    const uint64_t path_samples = shade_sample_count( sc.prm.path_samples, diffuse_intensity );
#include "acn_k_shade_path_loop.h"
                    bsum = group_sum< LPT >( bsum ) * F.get( TF_NORM );
                    if( writer )
                    {
                        V3 lum = F.get3( TF_LUM );
                        lum.x += bg.x * bsum; lum.y += bg.y * bsum; lum.z += bg.z * bsum;
                        fr_.set3( true, TF_LUM, lum );
                    }
                }
                fr_.publish();
            }

            /* end phase */
            if( setup ) pixel_add( accum, sc.flags, t.pixel, v_mld( ldc( t.Tc ), mine.get3( TF_LUM ) ) );
            ACN_LAP( PH_SHADE );
        }
    }
    /* persistent waves: G tasks per step, fetched fetch_batch at a time through the class's cursor */
    else for( ;; )
    {
        uint32_t base = 0;
        uint32_t got = range_take( fr, p_counts + QC_CUR_SHADE0 + cls, fetch_batch, n_tasks, ( uint32_t )G, &base );
        if( got == 0 ) break;
        uint32_t ti = base + grp;
        if( ( uint32_t )grp >= got ) continue;
        uint32_t slot = ( ( ElemP )( const void* )idx )[ ti ];
        if( LPT == 64 ) slot = __builtin_amdgcn_readfirstlane( slot );
        if( slot == ACN_INVALID ) continue;
        const DTask ACN_CONST& t = ( ( const DTask ACN_CONST* )tasks )[ slot ];
        const V3 pos = ldc( t.pos );   /* the origin of every ray of the task: stays in registers */
        const double diffuse_intensity = t.diffuse_intensity;
        const bool oren_nayar = t.on_b > 0;
        ACN_SHADE_TASK_SETUP( fr_, writer )
        uint64_t rv = t.rv;
        V3 lum = mk( 0, 0, 0 );   /* lum_l of scene.c:539, identical in all lanes of the group after each reduction */
        ACN_LAP( PH_FETCH );      /* diagnostic build: k_shade books 10 task fetch / set-up, 12 light set-up (cone cull, frame, root set),
                                     4 cap sample, 5 light hit, 6 Oren-Nayar, 7 occlusion, 8 queue appends and sums, 13 path set-up,
                                     9 path sample, 11 path transition hit; batched: the set-up of the tasks of a batch, one per lane */
        const uint64_t direct_samples = shade_sample_count( sc.prm.direct_samples, diffuse_intensity );
        NodeP light = &sc.nodes[ sc.light_root ];
        const int n_lights = light->child1;

        /* ---- direct light, scene.c:542-581 ---- */
        for( int li = 0; li < n_lights; li++ )
        {
            int light_idx = __builtin_amdgcn_readfirstlane( sc.elems[ light->child0 + li ] );
            NodeP light_src = &sc.nodes[ light_idx ];
            MatP light_mat = &sc.mats[ light_idx ];
            if( sub == 0 ) cnt.cost( ACN_F_FOV + ACN_F_FRAME );   /* per task and light: booked by one lane of the group */
            uint64_t skip;
            V3 light_color;
            double norm;
            ACN_SHADE_LIGHT_SETUP( fr_, writer )
            fr_.publish();
            const auto root_at = root_set< WAVE_LOOPS >( scp, sc.matter_root, skip );
            ACN_LAP( PH_LIGHT_SETUP );

#include "acn_k_shade_direct_loop.h"
            rv = lcg00_jump( rv, 2 * direct_samples );
            s = group_sum< LPT >( s );
            double f = s * norm;
            lum.x += light_color.x * f; lum.y += light_color.y * f; lum.z += light_color.z * f;
            ACN_LAP( PH_SHADE );
        }

        /* ---- path tracing, scene.c:584-621 ---- */
        if( sc.prm.path_samples && t.depth > 10 )
        {
            if( sub == 0 ) cnt.cost( ACN_F_FRAME );
            const uint64_t path_samples = shade_sample_count( sc.prm.path_samples, diffuse_intensity );
            const double norm = 2.0 / path_samples;
            const V3 bg = ld3( sc.prm.background_color );
            const double path_limit = shade_path_limit( sc.prm.max_path_length );
            ACN_SHADE_PATH_SETUP( fr_, writer )
            fr_.publish();
            ACN_LAP( PH_PATH_SETUP );
#include "acn_k_shade_path_loop.h"
            bsum = group_sum< LPT >( bsum ) * norm;
            lum.x += bg.x * bsum; lum.y += bg.y * bsum; lum.z += bg.z * bsum;
        }

        if( sub == 0 ) pixel_add( accum, sc.flags, t.pixel, v_mld( ldc( t.Tc ), lum ) );
        ACN_LAP( PH_SHADE );
    }
    chunk_close( cs + 0, hs_cap, kill_hs );
    chunk_close( cs + 1, hard_cap, kill_hp, p_counts + QS_DEAD_HP );
    chunk_close( cs + 2, child_cap, kill_ch, p_counts + QS_DEAD_C );
    wave_stat_add( p_counts + QS_HARD_SHADOW, n_hs );
    wave_stat_add( p_counts + QS_HARD_PATH, n_hp );
    wave_stat_add( p_counts + QS_CHILDREN, n_ch );
    ACN_PHASE_FLUSH( counters, 3 )
    wave_add_counters( counters, cnt );
}

/* body of acn_launch_shade<LPT>: shared by the four k_shade translation units */
#define ACN_DEFINE_LAUNCH_SHADE( NAME, LPT, CLS ) \
void NAME( KernelFlags f, const LevelQ& q, hipStream_t stream, const SceneArgs& s, unsigned long long* accum, unsigned long long* counters ) \
{ \
    acn_variant( f.count, f.prune, f.leaf_lights, [ & ]( auto C, auto P, auto L ) { \
        hipLaunchKernelGGL( ( k_shade< LPT, C.value, L.value, P.value > ), dim3( q.shade_grid ), dim3( 256 ), 0, stream, ACN_SCENE_ARGS_OF( s ), \
            ( const DTask* )q.tasks, ( const uint32_t* )q.idx[ CLS ], CLS, q.task_cap, q.fetch_shade * ( 64u / LPT ), q.children, q.child_cap, q.hard_shadow, \
            q.hard_path, q.hs_cap, q.hard_cap, q.counts, q.shard_rank, q.shard_world, accum, counters ); } ); \
}

#endif /* ACN_K_SHADE_H */
