/* acn_k_shade_direct_loop.h -- the direct-light loop of one task and light on the lanes of its group (scene.c:556-577), as text:
 * k_shade (acn_k_shade.h) includes it in the step of the plain form and in the sub-step of the batched form, so that the form a
 * change does not touch compiles from the same tokens as before.  No header: it is a piece of k_shade's body.
 * In scope where it is included: t (the DTask), pos, oren_nayar, light_src, light_idx, skip, root_at, direct_samples, and rv, the
 * state of the task's LCG stream the loop starts from; F is the task's frame.  It leaves the lane's partial sum in s. */
double s = 0;
/* ACN_SHARD_SAMPLES (shard_world > 1, level 0 only): this rank's share of the loop; sample j keeps its
 * place in the LCG stream and the normalisation above keeps the whole loop's n */
uint64_t j_lo = 0, j_hi = direct_samples;
uint64_t rv0 = rv;
if( shard_world > 1 )
{
    j_lo = direct_samples * shard_rank / shard_world; j_hi = direct_samples * ( shard_rank + 1 ) / shard_world;
    rv0 = lcg00_jump( rv, 2 * j_lo );
}
uint64_t rvj = lcg_jump_lane( rv0, sub );
for( uint64_t j = j_lo + sub; j < j_hi; j += LPT )
{
    ACN_TALLY( 0, true );   /* diagnostic build: lanes in a round of the direct-light loop */
    uint64_t r = rvj;
    rvj = lcg_stride< LPT >( rvj );
    cnt.inc( CNT_CAP_SAMPLE );
    cnt.cost( ACN_F_CAP_SAMPLE, ACN_T_CAP_SAMPLE );
    const V3 cap = shade_sphere_cap< WAVE_LOOPS >( &r, F.get( TF_CYL_HGT ) );
    const V3 out_d = m_mlv( frame_con( F ), cap );
    double weight = v_mlv( out_d, F.get3( TF_SURFACE_D ) );
    ACN_LAP( PH_M_LEAF );
    if( weight <= 0 ) continue;
    double a;
    if( LEAF_LIGHTS ) a = leaf_element_hit< false >( light_src, light_src->type, pos, out_d, nullptr, &cnt );
    else a = light_hit_call( sc, light_idx, pos, out_d, &cnt );
    ACN_LAP( PH_M_PAIR );
    if( a >= F3_INF ) continue;
    cnt.inc( CNT_SHADOW_RAY );
    ACN_LAP( PH_M_FRAME );
    uint32_t cand;   /* occ == 2: the machine elements left for k_hard_shadow */
    int occ = root_occluded_fast( scp, sc.matter_root, pos, out_d, a, skip, &cand, &cnt, root_at );
    ACN_LAP( PH_M_SIDE );
    if( occ == 1 ) continue;
    /* what the sample adds if it is not occluded (scene.c:569-574); the weight of a direct-light sample only scales its
     * colour: closed form (oren_nayar_weight_direct).  Computed behind the occlusion test: an occluded sample needs none
     * of it, and the test above holds no register for it */
    if( oren_nayar )
    {
        cnt.cost( ACN_F_OREN_NAYAR_DIRECT );
        weight = oren_nayar_weight_direct( weight, F.get( TF_SIN_I ), F.get( TF_COS_I ), F.get( TF_TAN_I ), F.get( TF_ON_A ), F.get( TF_ON_B ), out_d,
                                           F.get3( TF_SURFACE_D ), F.get3( TF_RAY_PRJ ) );
    }
    V3 hit_pos = ray_pos( pos, out_d, a );
    double diff_sqr = v_diff_sqr( hit_pos, F.get3( TF_LIGHT_POS ) );
    double local_intensity = ( diff_sqr > 0 ) ? ( F.get( TF_RADIANCE ) / diff_sqr ) : F3_MAG;
    double c = local_intensity * weight * F.get( TF_DIFF_I );
    if( cand == 0 ) { s += c; cnt.cost( ACN_F_DIRECT_TAIL ); }
    /* hard shadow rays: appended to the queue of k_hard_shadow, which adds the contribution itself if unoccluded */
    uint32_t hs = chunk_alloc( cs + 0, &p_counts[ QC_HARD_SHADOW ], cand != 0 );
    if( cand != 0 )
    {
        if( hs < hs_cap )
        {
            HardShadow& h = p_hard_shadow[ hs ];
            const V3 scale = F.get3( TF_SCALE );
            h.pos = pos; h.d = out_d; h.limit = a;
            h.contrib = mk( scale.x * c, scale.y * c, scale.z * c );
            h.pixel = t.pixel; h.pad = resume_record( cand );
            n_hs++;
        }
        else
        {
            atomicOr( sc_in.flags, ACN_FLAG_CHILD_OVERFLOW );
        }
    }
}
