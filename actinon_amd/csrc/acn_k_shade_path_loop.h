/* acn_k_shade_path_loop.h -- the path loop of one task on the lanes of its group (scene.c:596-621), as text: see
 * acn_k_shade_direct_loop.h.  In scope where it is included: t (the DTask), pos, oren_nayar, diffuse_intensity, path_samples,
 * path_limit, bg, and rv, the state of the task's LCG stream the loop starts from; F is the task's frame.  It leaves the lane's
 * share of the background sum in bsum. */
double bsum = 0;
uint64_t j_lo = 0, j_hi = path_samples;
uint64_t rv0 = rv;
if( shard_world > 1 )
{
    j_lo = path_samples * shard_rank / shard_world; j_hi = path_samples * ( shard_rank + 1 ) / shard_world;
    rv0 = lcg00_jump( rv, 2 * j_lo );
}
uint64_t rvj = lcg_jump_lane( rv0, sub );
for( uint64_t j = j_lo + sub; j < j_hi; j += LPT )
{
    ACN_TALLY( 2, true );   /* ... of the path loop */
    uint64_t r = rvj;
    rvj = lcg_stride< LPT >( rvj );
    cnt.inc( CNT_CAP_SAMPLE );
    cnt.cost( ACN_F_CAP_SAMPLE, ACN_T_CAP_SAMPLE );
    const V3 cap = shade_sphere_cap< WAVE_LOOPS >( &r, 1.0 );
    const V3 out_d = m_mlv( frame_con( F ), cap );
    double weight = v_mlv( out_d, F.get3( TF_SURFACE_D ) );
    bool live = weight > 0;
    double a = F3_INF;
    Trans trans;
    trans.exit_nor = mk( 0, 0, 0 ); trans.exit_obj = -1; trans.enter_obj = -1;
    bool hard = false;
    uint32_t machines = 0, inline_hits = 0;   /* candidate words of the in-line pass: what is left for the hard-ray kernels */
    if( live )
    {
        if( oren_nayar )
        {
            cnt.cost( ACN_F_OREN_NAYAR, ACN_T_OREN_NAYAR );
            weight = oren_nayar_weight_pre( weight, F.get( TF_THETA_I ), F.get( TF_SIN_I ), F.get( TF_COS_I ), F.get( TF_ON_A ), F.get( TF_ON_B ), out_d,
                                            F.get3( TF_SURFACE_D ), F.get3( TF_RAY_PRJ ) );
        }
        cnt.cost( ACN_F_PATH_TAIL );
        ACN_LAP( PH_COMPOUND );
        a = root_trans_hit_fast( scp, sc.matter_root, pos, out_d, &trans, &hard, &machines, &inline_hits, &cnt );
        ACN_LAP( PH_TAIL );
    }
    const double child_intensity = weight * diffuse_intensity;
    bool hit = live && !hard && a < sc.prm.max_path_length;
    if( live && !hard && !hit ) bsum += child_intensity;
    /* scene_s_lum of a hit with depth - 10 == 0 or too little intensity is zero (scene.c:430): such a hit is not
     * queued, and such a ray that needs the machine only needs a yes / no (see probe_push) */
    const bool dark = t.depth - 10 == 0 || child_intensity < sc.prm.trace_min_intensity;
    if( dark ) hit = false;
    const bool probe = hard && dark;
    if( probe ) { hard = false; cnt.inc( CNT_TRANS_RAY ); }   /* the compound_s_ray_trans_hit this probe stands for */
    /* a probe whose in-line elements already hit within the limit is occluded whatever the machines say: not written */
    const bool probe_open = probe && !( a <= path_limit );
    uint32_t ps = chunk_alloc( cs + 0, &p_counts[ QC_HARD_SHADOW ], probe_open );
    if( probe_open )
    {
        if( ps < hs_cap )
        {
            HardShadow& h = p_hard_shadow[ ps ];
            h.pos = pos; h.d = out_d; h.limit = path_limit;
            h.contrib = v_mld( F.get3( TF_SCALE ), v_mlf( bg, child_intensity ) );   /* k_hard_path's term for a miss */
            h.pixel = t.pixel; h.pad = resume_record( machines );
            n_hs++;
        }
        else
        {
            atomicOr( sc_in.flags, ACN_FLAG_CHILD_OVERFLOW );
        }
    }
    /* hard path rays: the transition hit is finished by k_hard_path */
    uint32_t hp = chunk_alloc( cs + 1, &p_counts[ QC_HARD_PATH ], hard );
    if( hard )
    {
        if( hp < hard_cap )
        {
            HardPath& h = p_hard_path[ hp ];
            h.pos = pos; h.d = out_d; h.T = F.get3( TF_SCALE ); h.intensity = child_intensity;
            h.depth = t.depth - 10; h.pixel = t.pixel;
            h.resume = resume_record( machines | inline_hits ); h.pad = 0;
            n_hp++;
        }
        else
        {
            atomicOr( sc_in.flags, ACN_FLAG_CHILD_OVERFLOW );
        }
    }
    /* the surviving path rays: the next level's queue */
    uint32_t csl = chunk_alloc( cs + 2, &p_counts[ QC_CHILDREN ], hit );
    if( hit )
    {
        if( csl < child_cap )
        {
            HitRec& c = p_children[ csl ];
            c.p = pos; c.d = out_d; c.offs = a; c.exit_nor = trans.exit_nor; c.T = F.get3( TF_SCALE );
            c.intensity = child_intensity;
            c.exit_obj = trans.exit_obj; c.enter_obj = trans.enter_obj;
            c.depth = t.depth - 10; c.pixel = t.pixel;
            n_ch++;
        }
        else
        {
            atomicOr( sc_in.flags, ACN_FLAG_CHILD_OVERFLOW );
        }
    }
}
